"""Reverse-KL training on a hidden-Markov-model target (HiddenMarkovTarget, NF_TARGET_HMM_NORMAL), 65 536 draws: K = 4 states,
normal emissions, one sequence of R = 1 024 rows, d = 28.  Per flow one JSON line:
  realnvp   cfg-2's coupling flow at this d (RealNVP, hidden [64, 64], 8 couplings)
  fullrank  a full-rank Gaussian at d = 28
Arm a: the device target (nf_elbo_step, asynchronous); arm b: the CLOSURE route (value_and_gradient with an ordinary torch `logp`
doing the log-space forward algorithm, R dependent logsumexp steps, autograd through all of them, plus adam_update).
*_ms -- ms per training step of the arm; a_launch_ms -- ms per "target_hmm" launch (HIP events around the launch, nf_prof_read, in
runs of their own); exp_per_launch -- the exponentials b_t(k) the launch evaluates (one per row, state and sample in each of the
forward sweep, the replay of all segments but the last and the reverse sweep), gexp_per_s that count over the launch time.  The
arms' timed loops alternate after a clock ramp of --ramp seconds; every figure is the median of --runs loops with the spread
(max - min) next to it.  The rows are also written to --out.
usage: python tools/bench_hmm_target.py [--runs 5] [--out profiles/hmm_target.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
from tools.bench_glm_targets import B1, B2, EPS, LR, timed  # noqa: E402

N, ROWS, K = 65536, 1024, 4


def model(nf, gen):
    """(HiddenMarkovTarget, the closure) of one four-regime normal series"""
    st = torch.cumsum((torch.rand(ROWS, generator=gen) < 0.05).long(), 0) % K
    x = (2.0 * st + 0.5 * torch.randn(ROWS, generator=gen)).float().cuda()
    d = K + K * K + 2 * K
    loc = [0.0] * (K + K * K) + [2.0 * k for k in range(K)] + [-0.7] * K  # the locations order the states
    tgt = nf.HiddenMarkovTarget("normal", x, K, prior_loc=loc, prior_scale=1.5)
    pm = torch.tensor(loc, device="cuda")[:, None]

    def logp(ys):  # (d, N) -> (N,): the same density up to its constant, in log space
        lpi = torch.log_softmax(ys[:K], 0)
        lP = torch.log_softmax(ys[K:K + K * K].reshape(K, K, -1), 1)
        mu, ls = ys[K + K * K:K + K * K + K], ys[K + K * K + K:]
        einv = torch.exp(-ls)
        la = None
        for t in range(ROWS):
            z = (x[t] - mu) * einv
            l = -0.5 * z * z - ls
            la = lpi + l if la is None else torch.logsumexp(la[:, None, :] + lP, 0) + l
        return torch.logsumexp(la, 0) - 0.5 * (((ys - pm) / 1.5) ** 2).sum(0)

    return tgt, logp, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ramp", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmm_target.json"))
    args = ap.parse_args()
    nf = load_package()
    lib = nf.load_library()
    tgt, logp, d = model(nf, torch.Generator().manual_seed(1))
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    L = nf._lib.NF_HMM_SEGMENT
    nseg = -(-ROWS // L)
    last = ROWS - (nseg - 1) * L  # rows of the last segment: recorded by the forward sweep, not replayed
    exps = N * K * (2 * ROWS + (ROWS - last))
    out = []
    for fname in ("realnvp", "fullrank"):
        flow = nf.realnvp(nf.MvNormal(d), (64, 64), 4, paramtype=torch.float32, seed=1) if fname == "realnvp" else nf.fullrank(nf.MvNormal(d), paramtype=torch.float32)
        theta0, re = flow.destructure()
        ctx = flow.ctx
        row = {"flow": fname + ("_cfg2_h64x8" if fname == "realnvp" else ""), "N": N, "d": d, "K": K, "rows": ROWS, "segment": L}
        fns = {}
        for arm in ("a", "b"):
            th = theta0.clone()
            if arm == "b":  # the closure route
                st, rng = nf.setup(nf.Adam(LR), th), nf.PhiloxRNG(7)

                def fn(th=th, st=st, rng=rng):
                    _, g = nf.value_and_gradient(nf.elbo_batch, re(th), logp, N, rng)
                    nf.update(nf.Adam(LR), st, th, g, want_norm=True)
            else:
                m, v, k = torch.zeros_like(th), torch.zeros_like(th), [0]

                def fn(th=th, m=m, v=v, k=k):
                    nf._lib.check(lib.nf_elbo_step(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), N, 7, k[0], LR, B1, B2, EPS, None, None))
                    k[0] += 1
            fns[arm] = fn
            fn()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.ramp:  # clock ramp
            fns["a"]()
        torch.cuda.synchronize()
        ms = {arm: [] for arm in fns}
        for _ in range(args.runs):  # the arms alternate
            ms["a"].append(timed(fns["a"]))
            ms["b"].append(timed(fns["b"], min_iters=2))
        for arm, t in ms.items():
            row[arm + "_ms"], row[arm + "_spread"] = round(statistics.median(t), 4), round(max(t) - min(t), 4)
        row["b_over_a"] = round(row["b_ms"] / row["a_ms"], 2)
        per = []  # the target launch alone, from events around it (runs of their own: the events perturb the step's timing)
        for _ in range(args.runs):
            nf._lib.check(lib.nf_prof_enable(ctx.ptr, 2))
            for _ in range(20):
                fns["a"]()
            t, cnt = C.c_double(0.0), C.c_int64(0)
            nf._lib.check(lib.nf_prof_read(ctx.ptr, b"target_hmm", C.byref(t), C.byref(cnt)))
            nf._lib.check(lib.nf_prof_enable(ctx.ptr, 0))
            assert cnt.value == 20, cnt.value
            per.append(t.value)
        med = statistics.median(per)
        row["a_launch_ms"], row["a_launch_spread"] = round(med, 5), round(max(per) - min(per), 5)
        row["exp_per_launch"], row["gexp_per_s"] = exps, round(exps / (med * 1e-3) / 1e9, 2) if med > 0 else None
        row["ns_per_row_and_sample"] = round(med * 1e6 / (ROWS * N), 6) if med > 0 else None
        print(json.dumps(row), flush=True)
        out.append(row)
        del flow, fns
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
