"""The float64 oracle's forward-KL value and gradient of a LARGE batch, summed over chunks of samples in worker processes.

oracle.nf_oracle.neg_loglik_value_and_grad solves a dense d x d system per sample and layer (it is independent of any closed-form
inverse Jacobian on purpose), about 5 ms per sample and core at d = 64 with 8 couplings; loss and gradient are sums over samples
scaled by 1 / n_global, so chunks of the batch add up exactly as the one call does up to float64 summation order.

Run as a script in a process of its own (no torch, no GPU: the workers are forked):
    python oracle_pool.py IN.npz OUT.npz      IN: kind, d, nlayers, hdims, theta, ys      OUT: loss, grad
"""
import os
import sys

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"  # one BLAS thread per worker; set before numpy loads
import numpy as np  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import nf_oracle as o  # noqa: E402

CHUNK = 512
_job = {}


def _chunk(lo):
    ys = _job["ys"][:, lo:lo + CHUNK]
    return o.neg_loglik_value_and_grad(_job["spec"], _job["theta"], np.ascontiguousarray(ys), n_global=_job["ys"].shape[1])


def neg_loglik_value_and_grad(spec, theta, ys, workers=None):
    import multiprocessing as mp

    _job.update(spec=spec, theta=theta, ys=ys)
    if workers is None:
        workers = min(16, len(os.sched_getaffinity(0)))
    starts = list(range(0, ys.shape[1], CHUNK))
    with mp.get_context("fork").Pool(workers) as pool:
        parts = pool.map(_chunk, starts, chunksize=1)
    return sum(p[0] for p in parts), np.sum([p[1] for p in parts], axis=0)


if __name__ == "__main__":
    z = np.load(sys.argv[1])
    spec = o.FlowSpec(str(z["kind"]), int(z["d"]), int(z["nlayers"]), tuple(int(h) for h in z["hdims"]))
    loss, grad = neg_loglik_value_and_grad(spec, z["theta"], z["ys"])
    np.savez(sys.argv[2], loss=loss, grad=grad)
