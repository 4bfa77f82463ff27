"""Reverse-KL training on the Gaussian-mixture target (MixtureTarget: K full-covariance components): per case one JSON line with
  mixture_ms        -- ms per "target_mixture" launch (HIP events around the launch, nf_prof_read) inside nf_elbo_step,
  mixture_roofline  -- its fraction of the fp32-MFMA roofline: 4 K d^2 N flop (two GEMMs per component) over 157.3 TFLOP/s,
  step_ms           -- ms per nf_elbo_step with the built-in target (asynchronous: no host read),
  closure_ms        -- ms per iteration of the CLOSURE route on the same box and in the same process: value_and_gradient with an
                       ordinary torch `logp` doing the same K matmuls plus torch.logsumexp (library forward that keeps its tape,
                       torch autograd for the score, library pullback) plus adam_update -- the only way to train on such a
                       target without the kind.
The two timed loops are interleaved (step, closure, step, closure, ...) after a clock ramp of --ramp seconds; every figure is the
median of --runs loops, with the spread (max - min) next to it.
Cases: (a) the cfg-2 flow (RealNVP d = 64, hidden [64, 64], 8 couplings, 65 536 samples) on K = 16 components, (b) the cfg-3 flow
(NSF d = 32, K = 8, 131 072 samples) on K = 8 components.
usage: python tools/bench_mixture_target.py [--runs 5] [--case a,b] [--out profiles/mixture_target.json]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
MFMA_F32_TFLOPS = 157.3


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


def mixture(nf, d, K, gen):
    """Sigma_k = Q diag(lambda) Q', lambda in [0.5, 2]; means 3 randn(d) / sqrt(d); weights uniform in [0.5, 1.5], normalised"""
    Sig = []
    for _ in range(K):
        Q, _ = torch.linalg.qr(torch.randn(d, d, generator=gen, dtype=torch.float64))
        S = (Q * (0.5 + 1.5 * torch.rand(d, generator=gen, dtype=torch.float64))) @ Q.T
        Sig.append(0.5 * (S + S.T))
    mus = 3.0 * torch.randn(K, d, generator=gen, dtype=torch.float64) / math.sqrt(d)
    w = 0.5 + torch.rand(K, generator=gen, dtype=torch.float64)
    tgt = nf.MixtureTarget((w / w.sum()).float().cuda(), mus.float().cuda(), torch.stack(Sig).float().cuda())
    W = tgt.A.reshape(tgt.K, d, d)
    mbar, b, c = tgt.p0[:d], tgt.p0[d:d + tgt.K * d].reshape(tgt.K, d), tgt.p0[d + tgt.K * d:]

    def logp(ys):  # (d, N) -> (N,): the same K matmuls, then torch.logsumexp over the components
        u = torch.matmul(W, ys - mbar[:, None]) - b[:, :, None]
        return torch.logsumexp(c[:, None] - 0.5 * (u * u).sum(1), dim=0)

    return tgt, logp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ramp", type=float, default=1.0)
    ap.add_argument("--case", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    nf = load_package()
    lib = nf.load_library()
    q = lambda d: nf.MvNormal(d)  # noqa: E731
    f32 = torch.float32
    gen = torch.Generator().manual_seed(1)
    cases = [
        ("a_cfg2_realnvp_d64_h64x8", 16, lambda: nf.realnvp(q(64), (64, 64), 4, paramtype=f32, seed=1), 65536),
        ("b_cfg3_nsf_d32_k8x8", 8, lambda: nf.nsf(q(32), (32, 32), 8, 5.0, 4, paramtype=f32, seed=1), 131072),
    ]
    want = [c for c in args.case.split(",") if c]
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rows_out = []
    for name, K, make, n in cases:
        if want and name[0] not in want:
            continue
        flow = make()
        d = flow.dist.d
        tgt, torch_logp = mixture(nf, d, K, gen)
        theta0, re = flow.destructure()
        row = {"flow": name, "target": f"gaussmix_K{K}", "N": n, "d": d, "K": K}
        ctx = flow.ctx
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
        nf._lib.check(lib.nf_prof_read(ctx.ptr, b"target_mixture", C.byref(ms), C.byref(cnt)))
        nf._lib.check(lib.nf_prof_enable(ctx.ptr, 0))
        row["mixture_ms"], row["mixture_launches"] = round(ms.value, 5), cnt.value
        flop = 4.0 * K * d * d * n
        row["mixture_gflop"] = round(flop / 1e9, 3)
        row["mixture_roofline"] = round(flop / (ms.value * 1e-3) / (MFMA_F32_TFLOPS * 1e12), 4) if ms.value > 0 else None
        print(json.dumps(row), flush=True)
        rows_out.append(row)
        del flow, th, m, v, th2
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/bench_mixture_target.py", "runs": args.runs, "ramp_s": args.ramp, "rows": rows_out}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
