"""Reverse-KL training on the one-hidden-layer Bayesian neural-network target (BNNRegressionTarget, 1 024 data rows with row
weights, 65 536 samples):
  cfg2      the cfg-2 flow (RealNVP d = 64, hidden [64, 64], 8 couplings) with H = 3 hidden units over p = 20 features,
  fullrank  the full-rank Gaussian family at d = 241 with H = 16 hidden units over p = 14 features.
Per case one JSON line with
  bnn_ms            -- ms per "target_bnn" launch (HIP events around the launch, nf_prof_read) inside nf_elbo_step,
  bnn_roofline      -- its fraction of the fp32-MFMA figure on 4 rows H p N flop (the two GEMMs of the model; the kernel itself runs
                       GEMM 1 twice, which this figure does not credit) over 157.3 TFLOP/s,
  step_ms           -- ms per nf_elbo_step with the built-in target (asynchronous: no host read),
  closure_ms        -- ms per iteration of the CLOSURE route on the same box and in the same process: value_and_gradient with an
                       ordinary torch `logp` doing the same arithmetic (matmul, torch.tanh, the output layer, the Gaussian row
                       function; library forward that keeps its tape, torch autograd for the score, library pullback) plus
                       adam_update -- how such a posterior is trained without the kind.
The two timed loops are interleaved (step, closure, step, closure, ...) after a clock ramp of --ramp seconds; every figure is the
median of --runs loops, with the spread (max - min) next to it.  The rows are also written to --out as one JSON list.
usage: python tools/bench_bnn_target.py [--runs 5] [--case cfg2,fullrank] [--out profiles/bnn_target.json]"""
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
SIGMA_HIDDEN, SIGMA_OUT, NOISE = 3.0, 2.0, 0.5


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


def torch_form(tgt):
    """the torch closure of the ("normal") target from its own device buffers: the same matmul, tanh, output layer and row function"""
    rows, p, H = tgt.rows, tgt.p, tgt.n_hidden
    X, scl, off, wt = tgt.A, tgt.p0[:rows], tgt.p0[rows:2 * rows], tgt.p0[2 * rows:3 * rows]
    c0, ph, po = (float(x) for x in tgt.p0[3 * rows + 1:3 * rows + 4])
    HP = H * p

    def logp(ys):  # (d, N) -> (N,)
        n = ys.shape[1]
        a = torch.tanh(X @ ys[:HP].reshape(H, p, n))                      # [H, rows, N]
        f = (a * ys[HP:HP + H].unsqueeze(1)).sum(0) + ys[HP + H].unsqueeze(0)  # [rows, N]
        u = scl[:, None] * f + off[:, None]
        return (wt[:, None] * (-0.5 * u * u)).sum(0) - 0.5 * ph * (ys[:HP] * ys[:HP]).sum(0) - 0.5 * po * (ys[HP:] * ys[HP:]).sum(0) + c0

    return logp


def make_target(nf, H, p, rows, gen):
    X = torch.randn(rows, p, generator=gen, dtype=torch.float64) / math.sqrt(p)
    X[:, 0] = 1.0
    t = torch.randn(rows, generator=gen, dtype=torch.float64)
    w = 0.5 + torch.rand(rows, generator=gen, dtype=torch.float64)
    tgt = nf.BNNRegressionTarget(X.float().cuda(), t.float().cuda(), H, noise_sigma=NOISE, weights=w.float().cuda(),
                                 prior_sigma_hidden=SIGMA_HIDDEN, prior_sigma_out=SIGMA_OUT)
    return tgt, torch_form(tgt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ramp", type=float, default=1.0)
    ap.add_argument("--case", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bnn_target.json"))
    args = ap.parse_args()
    nf = load_package()
    lib = nf.load_library()
    gen = torch.Generator().manual_seed(1)
    rows, n = 1024, 65536
    cases = [("cfg2", "cfg2_realnvp_d64_h64x8", 3, 20, lambda d: nf.realnvp(nf.MvNormal(d), (64, 64), 4, paramtype=torch.float32, seed=1)),
             ("fullrank", "fullrank_d241", 16, 14, lambda d: nf.fullrank(nf.MvNormal(d), paramtype=torch.float32))]
    want = [c for c in args.case.split(",") if c]
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = []
    for cname, fname, H, p, make_flow in cases:
        if want and cname not in want:
            continue
        d = H * (p + 1) + 1
        flow = make_flow(d)
        tgt, torch_logp = make_target(nf, H, p, rows, gen)
        theta0, re = flow.destructure()
        row = {"flow": fname, "target": f"bnn_normal_H{H}_p{p}_n{rows}", "N": n, "d": d, "rows": rows}
        ctx = flow.ctx
        # the closure and the kind compute the same density (a few points, before anything is timed)
        ys = torch.randn(d, 8, device="cuda")
        dev_lp = nf.target_logp(tgt, ys)
        row["closure_vs_kind_max_rel"] = float(((torch_logp(ys) - dev_lp).abs() / dev_lp.abs()).max())
        th = theta0.clone()
        m, v = torch.zeros_like(th), torch.zeros_like(th)
        k = [0]

        def step():
            nf._lib.check(lib.nf_elbo_step(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, 7, k[0], LR, B1, B2, EPS, None, None))
            k[0] += 1

        th2 = theta0.clone()
        st = nf.setup(nf.Adam(LR), th2)
        rng = nf.PhiloxRNG(7)

        def closure():
            _, g = nf.value_and_gradient(nf.elbo_batch, re(th2), torch_logp, n, rng)
            nf.update(nf.Adam(LR), st, th2, g, want_norm=True)

        step()
        closure()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.ramp:  # clock ramp
            step()
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(args.runs):  # interleaved A/B
            a.append(timed(step))
            b.append(timed(closure))
        row["step_ms"], row["step_spread"] = round(statistics.median(a), 4), round(max(a) - min(a), 4)
        row["closure_ms"], row["closure_spread"] = round(statistics.median(b), 4), round(max(b) - min(b), 4)
        row["closure_over_step"] = round(row["closure_ms"] / row["step_ms"], 3)
        # the target launch alone, from events around it (a run of its own: the events perturb the step's timing)
        nf._lib.check(lib.nf_prof_enable(ctx.ptr, 2))
        for _ in range(20):
            step()
        torch.cuda.synchronize()
        ms, cnt = C.c_double(0.0), C.c_int64(0)
        nf._lib.check(lib.nf_prof_read(ctx.ptr, b"target_bnn", C.byref(ms), C.byref(cnt)))
        nf._lib.check(lib.nf_prof_enable(ctx.ptr, 0))
        row["bnn_ms"], row["bnn_launches"] = round(ms.value, 5), cnt.value
        flop = 4.0 * rows * H * p * n
        row["bnn_gflop"] = round(flop / 1e9, 3)
        row["bnn_roofline"] = round(flop / (ms.value * 1e-3) / (MFMA_F32_TFLOPS * 1e12), 4) if ms.value > 0 else None
        print(json.dumps(row), flush=True)
        out.append(row)
        del flow, th, m, v, th2
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
