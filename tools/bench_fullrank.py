"""Full-rank Gaussian VI (NF_KIND_FULLRANK, y = mu + L x) on the library's own posterior targets: ms per nf_elbo_step at
d = 64 and d = 256, N = 65 536 draws, Float32, on logistic regression with 1 024 rows and on a dense Gaussian.  Per case one
JSON line with
  step_ms        -- ms per nf_elbo_step (asynchronous: no host read),
  torch_ms       -- ms per iteration of the same step in torch on the same GPU and in the same process: mu + x @ tril(L).T, the
                    torch `logp` closure of the target, autograd, torch.optim.Adam,
  meanfield_ms   -- ms per iteration of the DIAGONAL family (`meanfield`) on the same target: the closure route (library forward
                    with its tape, the target's autograd node for the score, library pullback) plus adam_update,
  gemm_ms, bwd_ms -- HIP-event time of the two new kernels (k_fr_gemm forward, k_fr_bwd) inside the step, each as a fraction of the
                    fp32-MFMA figure (N d^2 flop: the triangular half of 2 N d^2) and of the HBM copy figure (8 N d bytes
                    through the forward, 8 N d + the slabs through the reverse kernel) DESIGN.md section 4 quotes.
The three timed loops are interleaved after a clock ramp of --ramp seconds; every figure is the median of --runs loops with the
spread (max - min) next to it.  The rows are also written to --out as one JSON list.
usage: python tools/bench_fullrank.py [--runs 5] [--out profiles/fullrank.json]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
MFMA_F32_TFLOPS = 157.3
HBM_COPY_TBS = 4.7
SIGMA = 2.0


def timed(fn, seconds=0.25, min_iters=5):
    """ms per call over a loop sized to last about `seconds`"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    iters = max(min_iters, min(2000, int(seconds / max(time.perf_counter() - t0, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def logreg(nf, d, rows, gen):
    X = torch.randn(rows, d, generator=gen, dtype=torch.float64) / math.sqrt(d)
    t = torch.randint(0, 2, (rows,), generator=gen)
    tgt = nf.LogisticRegressionTarget(X.float().cuda(), t.cuda(), prior_sigma=SIGMA)
    A, c = tgt.A, -0.5 * d * math.log(2 * math.pi * SIGMA * SIGMA)

    def logp(ys):  # (d, N) -> (N,)
        return torch.nn.functional.logsigmoid(A @ ys).sum(0) - (ys * ys).sum(0) / (2 * SIGMA * SIGMA) + c

    return tgt, logp


def dense_gauss(nf, d, rows, gen):
    Q, _ = torch.linalg.qr(torch.randn(d, d, generator=gen, dtype=torch.float64))
    Sigma = (Q * (0.5 + 1.5 * torch.rand(d, generator=gen, dtype=torch.float64))) @ Q.T
    mu = 0.5 * torch.randn(d, generator=gen, dtype=torch.float64)
    tgt = nf.MvNormalTarget(mu.float().cuda(), (0.5 * (Sigma + Sigma.T)).float().cuda())
    W, m, c = tgt.W, tgt.mu, -0.5 * d * math.log(2 * math.pi) + tgt.logdet_w

    def logp(ys):
        u = W @ (ys - m[:, None])
        return c - 0.5 * (u * u).sum(0)

    return tgt, logp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ramp", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fullrank.json"))
    args = ap.parse_args()
    nf = load_package()
    lib = nf.load_library()
    gen = torch.Generator().manual_seed(1)
    rows, n = 1024, 65536
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = []
    for d in (64, 256):
        for tname, make_tgt in (("logreg", logreg), ("densegauss", dense_gauss)):
            tgt, torch_logp = make_tgt(nf, d, rows, gen)
            flow = nf.fullrank(nf.MvNormal(d), paramtype=torch.float32)
            ctx = flow.ctx
            row = {"flow": "fullrank", "target": f"{tname}_n{rows}" if tname == "logreg" else tname, "N": n, "d": d}
            th = flow.theta.clone()
            m, v = torch.zeros_like(th), torch.zeros_like(th)
            k = [0]

            def step():
                nf._lib.check(lib.nf_elbo_step(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, 7, k[0], LR, B1, B2, EPS, None, None))
                k[0] += 1

            # the same step in torch
            mu_t = torch.zeros(d, device="cuda", requires_grad=True)
            L_t = torch.eye(d, device="cuda", requires_grad=True)
            opt = torch.optim.Adam([mu_t, L_t], lr=LR, betas=(B1, B2), eps=EPS)
            c0 = -0.5 * d * math.log(2 * math.pi)

            def torch_step():
                x = torch.randn(n, d, device="cuda")
                Lt = torch.tril(L_t)
                y = mu_t + x @ Lt.T
                elbo = torch_logp(y.T) - (c0 - 0.5 * (x * x).sum(1)) + torch.log(torch.abs(torch.diagonal(Lt))).sum()
                opt.zero_grad(set_to_none=True)
                (-elbo.mean()).backward()
                opt.step()

            # the diagonal family on the same target: the closure route
            mf = nf.meanfield(nf.MvNormal(d), paramtype=torch.float32)
            th2, re2 = mf.destructure()
            st = nf.setup(nf.Adam(LR), th2)
            rng = nf.PhiloxRNG(7)

            def meanfield_step():
                _, g = nf.value_and_gradient(nf.elbo_batch, re2(th2), tgt, n, rng)
                nf.update(nf.Adam(LR), st, th2, g, want_norm=True)

            step()
            torch_step()
            meanfield_step()
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < args.ramp:  # clock ramp
                step()
            torch.cuda.synchronize()
            a, b, c = [], [], []
            for _ in range(args.runs):  # interleaved
                a.append(timed(step))
                b.append(timed(torch_step))
                c.append(timed(meanfield_step))
            for key, vals in (("step", a), ("torch", b), ("meanfield", c)):
                row[key + "_ms"], row[key + "_spread"] = round(statistics.median(vals), 4), round(max(vals) - min(vals), 4)
            row["torch_over_step"] = round(row["torch_ms"] / row["step_ms"], 3)
            # the two new kernels alone, from events around them (a run of its own: the events perturb the step's timing)
            nf._lib.check(lib.nf_prof_enable(ctx.ptr, 2))
            for _ in range(20):
                step()
            torch.cuda.synchronize()
            flop = float(n) * d * d
            grid = min((n + 31) // 32, torch.cuda.get_device_properties(0).multi_processor_count)
            traffic = {"fr_gemm": 8.0 * n * d, "fr_bwd": 8.0 * n * d + 4.0 * grid * (d + d * d)}
            for name, key in ((b"fr_gemm", "gemm"), (b"fr_bwd", "bwd"), (b"target_linpred", "target"), (b"reduce_slabs", "reduce")):
                ms, cnt = C.c_double(0.0), C.c_int64(0)
                nf._lib.check(lib.nf_prof_read(ctx.ptr, name, C.byref(ms), C.byref(cnt)))
                row[key + "_ms"] = round(ms.value, 5)
                if name.decode() in traffic and ms.value > 0:
                    row[key + "_mfma_fraction"] = round(flop / (ms.value * 1e-3) / (MFMA_F32_TFLOPS * 1e12), 4)
                    row[key + "_hbm_copy_fraction"] = round(traffic[name.decode()] / (ms.value * 1e-3) / (HBM_COPY_TBS * 1e12), 4)
            nf._lib.check(lib.nf_prof_enable(ctx.ptr, 0))
            row["gflop_per_kernel"] = round(flop / 1e9, 3)
            print(json.dumps(row), flush=True)
            out.append(row)
            del flow, th, m, v, th2, mu_t, L_t, opt
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
