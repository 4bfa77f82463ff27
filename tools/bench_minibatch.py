"""Row-minibatch ELBO steps against full-data steps on GLMTarget("logit") with R = 131 072 rows, 65 536 draws:
  flows   cfg2      the cfg-2 flow (RealNVP d = 64, hidden [64, 64], 8 couplings),
          fullrank  the full-rank Gaussian family at d = 256.
Per flow one JSON line with, in ms per nf_elbo_step (asynchronous: no host read),
  full_step_ms       -- (a) the full target, all R rows in every step,
  minibatch_step_ms  -- (b) MinibatchTarget with m = 1 024: nf_target_minibatch + nf_elbo_step, a new batch every step,
  plain_step_ms      -- (c) a plain 1 024-row GLMTarget (the first 1 024 rows): the code path without the wrapper,
  gather_ms          -- the "target_minibatch" launch alone (HIP events around it, nf_prof_read), gather_bytes = what it moves
                        (the m rows and their per-row values read and written, the fixed segments copied, the indices) and
                        gather_roofline = that over the 4.7 TB/s HBM copy figure of DESIGN section 4,
  call_ms            -- the host's time in one nf_target_minibatch call (the library call the wrapper adds),
  minibatch_minus_plain_ms against gather_ms + call_ms: what the wrapper costs and whether the launch and the call explain it.
The timed loops are interleaved (a, b, c, a, ...) after a clock ramp of --ramp seconds; every figure is the median of --runs loops
with the spread (max - min) next to it.
With --train SECONDS: -ELBO on the FULL target over 16 384 fixed draws after the same wall time of training from the same start,
(a) on the full target and (b) on the minibatch, lr 1e-3, n = 4 096 draws per step: a report, not a threshold.
usage: python tools/bench_minibatch.py [--runs 5] [--case cfg2,fullrank] [--train 3] [--out profiles/minibatch_target.json]"""
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
HBM_COPY_TBS = 4.7
SIGMA = 2.0
ROWS, BATCH, N = 131072, 1024, 65536
N_TRAIN, N_EVAL = 4096, 16384


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ramp", type=float, default=1.0)
    ap.add_argument("--case", default="")
    ap.add_argument("--train", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minibatch_target.json"))
    args = ap.parse_args()
    nf = load_package()
    lib = nf.load_library()
    gen = torch.Generator().manual_seed(1)
    flows = [("cfg2", "cfg2_realnvp_d64_h64x8", 64, lambda d: nf.realnvp(nf.MvNormal(d), (64, 64), 4, paramtype=torch.float32, seed=1)),
             ("fullrank", "fullrank_d256", 256, lambda d: nf.fullrank(nf.MvNormal(d), paramtype=torch.float32))]
    want = [c for c in args.case.split(",") if c]
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = []
    for cname, fname, d, make_flow in flows:
        if want and cname not in want:
            continue
        flow = make_flow(d)
        X = torch.randn(ROWS, d, generator=gen) / math.sqrt(d)
        beta = torch.randn(d, generator=gen)
        t = torch.where(torch.rand(ROWS, generator=gen) < torch.sigmoid(X @ beta), 1.0, -1.0)
        A = (X * t[:, None]).cuda()  # the labels folded into the rows: phi = log sigmoid(t x . z)
        full = nf.GLMTarget("logit", A, prior_sigma=SIGMA)
        mb = nf.MinibatchTarget(full, BATCH, seed=3)
        plain = nf.GLMTarget("logit", A[:BATCH].clone(), prior_sigma=SIGMA)
        theta0, re = flow.destructure()
        ctx = flow.ctx
        row = {"flow": fname, "target": f"glm_logit_p{d}", "N": N, "d": d, "rows": ROWS, "batch_rows": BATCH}

        def stepper(target, n, resample=False):
            th = theta0.clone()
            m, v = torch.zeros_like(th), torch.zeros_like(th)
            k = [0]

            def step():
                if resample:
                    target.resample(k[0])
                nf._lib.check(lib.nf_elbo_step(ctx.ptr, C.byref(flow.desc), C.byref(target.c), vp(th), vp(m), vp(v), n, 7, k[0], LR, B1, B2, EPS, None, None))
                k[0] += 1

            return step, (th, m, v)

        a_step, keep_a = stepper(full, N)
        b_step, keep_b = stepper(mb, N, resample=True)
        c_step, keep_c = stepper(plain, N)
        a_step(), b_step(), c_step()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.ramp:  # clock ramp
            c_step()
        torch.cuda.synchronize()
        ta, tb, tc = [], [], []
        for _ in range(args.runs):  # interleaved
            ta.append(timed(a_step))
            tb.append(timed(b_step))
            tc.append(timed(c_step))
        for key, ts in (("full", ta), ("minibatch", tb), ("plain", tc)):
            row[key + "_step_ms"], row[key + "_step_spread"] = round(statistics.median(ts), 4), round(max(ts) - min(ts), 4)
        row["full_over_minibatch"] = round(row["full_step_ms"] / row["minibatch_step_ms"], 2)
        row["minibatch_minus_plain_ms"] = round(row["minibatch_step_ms"] - row["plain_step_ms"], 4)
        # the gather launch alone, from events around it (a run of its own: the events perturb the step's timing)
        nf._lib.check(lib.nf_prof_enable(ctx.ptr, 2))
        for s in range(20):
            mb.resample(s)
        torch.cuda.synchronize()
        ms, cnt = C.c_double(0.0), C.c_int64(0)
        nf._lib.check(lib.nf_prof_read(ctx.ptr, b"target_minibatch", C.byref(ms), C.byref(cnt)))
        nf._lib.check(lib.nf_prof_enable(ctx.ptr, 0))
        row["gather_ms"], row["gather_launches"] = round(ms.value, 5), cnt.value
        es = 4
        row["gather_bytes"] = 2 * BATCH * d * es + 2 * 2 * BATCH * es + 2 * (d + 2) * es + BATCH * 4
        row["gather_roofline"] = round(row["gather_bytes"] / (row["gather_ms"] * 1e-3) / (HBM_COPY_TBS * 1e12), 4) if row["gather_ms"] > 0 else None
        # the host's time in the call (the launch is asynchronous)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(200):
            mb.resample(s)
        row["call_ms"] = round((time.perf_counter() - t0) * 1e3 / 200, 5)
        torch.cuda.synchronize()
        row["explained_ms"] = round(row["gather_ms"] + row["call_ms"], 5)
        if args.train > 0:
            xs = nf.device_specific_rand(nf.PhiloxRNG(99), flow.dist, N_EVAL, device=theta0.device, dtype=theta0.dtype)
            row["neg_elbo_full_at_start"] = round(-nf.elbo_batch(re(theta0), full, xs), 4)
            for key, target, resample in (("full", full, False), ("minibatch", mb, True)):
                step, (th, _, _) = stepper(target, N_TRAIN, resample)
                step()
                torch.cuda.synchronize()
                steps, t0 = 1, time.perf_counter()
                while time.perf_counter() - t0 < args.train:
                    for _ in range(8):
                        step()
                    torch.cuda.synchronize()
                    steps += 8
                row[f"train_{key}_steps"], row[f"train_{key}_seconds"] = steps, round(time.perf_counter() - t0, 3)
                row[f"train_{key}_neg_elbo_full"] = round(-nf.elbo_batch(re(th), full, xs), 4)
            row["train_lr"], row["train_n"], row["eval_draws"] = LR, N_TRAIN, N_EVAL
        print(json.dumps(row), flush=True)
        out.append(row)
        del flow, keep_a, keep_b, keep_c, full, mb, plain, A
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
