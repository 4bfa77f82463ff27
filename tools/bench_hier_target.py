"""Reverse-KL training on the hierarchical GLM targets (HierarchicalGLMTarget: p = 56 coefficients, 48 of them in G = 8 groups with
learned log-scales, 1 024 data rows; logit and poisson families) with the cfg-2 flow (RealNVP d = 64, hidden [64, 64], 8 couplings,
65 536 samples): per case one JSON line with
  step_ms / linpred_ms          -- ms per nf_elbo_step on the hierarchical target and per "target_linpred" launch inside it (HIP events
                                   around the launch, nf_prof_read, in a run of its own),
  linpred_roofline              -- the launch's fraction of the fp32-MFMA roofline: 4 r d N flop (two GEMMs) over 157.3 TFLOP/s,
  glm_step_ms / glm_linpred_ms  -- the same flow and the same rows (A with its zero tau-columns) on the matching GLMTarget with one
                                   N(0, sigma^2 I) prior: what the structured prior's epilogue costs,
  closure_ms                    -- ms per iteration of the CLOSURE route: value_and_gradient with an ordinary torch `logp` doing the
                                   same arithmetic (library forward that keeps its tape, torch autograd for the score, library
                                   pullback) plus adam_update -- how a hierarchical posterior is trained without the kinds,
  fullrank_step_ms              -- ms per nf_elbo_step of the full-rank Gaussian family on the same target.
The timed loops are interleaved (hier, glm, closure, fullrank, hier, ...) after a clock ramp of --ramp seconds; every figure is the
median of --runs loops, with the spread (max - min) next to it.  With --out the rows are also written there as one JSON list.
usage: python tools/bench_hier_target.py [--runs 5] [--case logit,poisson] [--out hier_target.json]"""
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
SIGMA = 2.0
P, G, ROWS, N = 56, 8, 1024, 65536
PHI = {"logit": torch.nn.functional.logsigmoid, "poisson": lambda u: -torch.exp(u)}


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


def make_targets(nf, family, gen):
    """the hierarchical target, the GLM target over the same rows, and the torch closure of the hierarchical density"""
    X = torch.randn(ROWS, P, generator=gen, dtype=torch.float64) / math.sqrt(P)
    off = 0.3 * torch.randn(ROWS, generator=gen, dtype=torch.float64)
    w = 0.5 + torch.rand(ROWS, generator=gen, dtype=torch.float64)
    lin = 0.3 * torch.randn(P, generator=gen, dtype=torch.float64)
    groups = torch.cat([torch.full((P - 6 * G,), -1), torch.arange(G).repeat_interleave(6)])  # 8 fixed-scale coefficients, 8 groups of 6
    hyper = ["halfcauchy", "halfnormal", "lognormal", "halfcauchy"] * 2
    f = lambda t: t.float().cuda()
    hier = nf.HierarchicalGLMTarget(family, f(X), groups.cuda(), G, f(off), f(w), f(lin), fixed_sigma=SIGMA, hyper=hyper, hyper_scale=1.5)
    glm = nf.GLMTarget(family, hier.A, f(off), f(w), hier.p0[:P + G].clone(), prior_sigma=SIGMA)
    # the closure: the same buffers, torch arithmetic
    d = P + G
    A, p0 = hier.A, hier.p0
    linv, offv, wtv, c = p0[:d], p0[d:d + ROWS], p0[d + ROWS:d + 2 * ROWS], float(p0[d + 2 * ROWS + 1])
    grouped = (groups >= 0).cuda()
    gi = groups.clamp(min=0).cuda()
    isd2 = (p0[d + 2 * ROWS + 2 + P:d + 2 * ROWS + 2 + 2 * P] ** 2)[:, None]
    at = d + 2 * ROWS + 2 + 2 * P
    hm, his = p0[at:at + G][:, None], p0[at + G:at + 2 * G][:, None]
    hk = [int(k) for k in p0[at + 2 * G:at + 3 * G].tolist()]
    phi = PHI[family]

    def logp(ys):  # (d, N) -> (N,)
        beta, tau = ys[:P], ys[P:]
        u = A @ ys + offv[:, None]
        om = torch.where(grouped[:, None], torch.exp(-2.0 * tau[gi]), isd2)
        x = tau - hm
        h = torch.stack([-0.5 * (x[g] * his[g]) ** 2 if hk[g] == 0 else -0.5 * torch.exp(2.0 * x[g]) if hk[g] == 1
                         else -torch.nn.functional.softplus(2.0 * x[g]) for g in range(G)])
        return (wtv[:, None] * phi(u)).sum(0) + linv @ ys - 0.5 * (beta * beta * om).sum(0) + h.sum(0) + c

    return hier, glm, logp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ramp", type=float, default=1.0)
    ap.add_argument("--case", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    nf = load_package()
    lib = nf.load_library()
    gen = torch.Generator().manual_seed(1)
    d = P + G
    want = [c for c in args.case.split(",") if c]
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = []
    for family in ("logit", "poisson"):
        if want and family not in want:
            continue
        flow = nf.realnvp(nf.MvNormal(d), (64, 64), 4, paramtype=torch.float32, seed=1)
        flow = flow.with_theta(flow.theta * 0.3)  # the log-scales start within a few units
        full = nf.fullrank(nf.MvNormal(d), paramtype=torch.float32)
        hier, glm, torch_logp = make_targets(nf, family, gen)
        theta0, re = flow.destructure()
        row = {"flow": "cfg2_realnvp_d64_h64x8", "target": f"hier_{family}_p{P}_G{G}_n{ROWS}", "N": N, "d": d, "rows": ROWS}

        def stepper(fl, tgt):
            th = fl.theta.clone()
            m, v = torch.zeros_like(th), torch.zeros_like(th)
            k = [0]

            def step():
                nf._lib.check(lib.nf_elbo_step(fl.ctx.ptr, C.byref(fl.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), N, 7, k[0], LR, B1, B2, EPS, None, None))
                k[0] += 1

            return step

        steps = {"step": stepper(flow, hier), "glm_step": stepper(flow, glm), "fullrank_step": stepper(full, hier)}
        th2 = theta0.clone()
        st = nf.setup(nf.Adam(LR), th2)
        rng = nf.PhiloxRNG(7)

        def closure():
            _, g = nf.value_and_gradient(nf.elbo_batch, re(th2), torch_logp, N, rng)
            nf.update(nf.Adam(LR), st, th2, g, want_norm=True)

        steps["closure"] = closure
        for fn in steps.values():
            fn()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.ramp:  # clock ramp
            steps["step"]()
        torch.cuda.synchronize()
        times = {k: [] for k in steps}
        for _ in range(args.runs):  # interleaved
            for k, fn in steps.items():
                times[k].append(timed(fn))
        for k, v in times.items():
            row[k + "_ms"], row[k + "_spread"] = round(statistics.median(v), 4), round(max(v) - min(v), 4)
        row["closure_over_step"] = round(row["closure_ms"] / row["step_ms"], 3)
        # the target launches alone, from events around them (runs of their own: the events perturb the step's timing)
        for key, name in (("linpred_ms", "step"), ("glm_linpred_ms", "glm_step")):
            nf._lib.check(lib.nf_prof_enable(flow.ctx.ptr, 2))
            for _ in range(20):
                steps[name]()
            torch.cuda.synchronize()
            ms, cnt = C.c_double(0.0), C.c_int64(0)
            nf._lib.check(lib.nf_prof_read(flow.ctx.ptr, b"target_linpred", C.byref(ms), C.byref(cnt)))
            nf._lib.check(lib.nf_prof_enable(flow.ctx.ptr, 0))
            row[key] = round(ms.value, 5)
        flop = 4.0 * ROWS * d * N
        row["linpred_gflop"] = round(flop / 1e9, 3)
        row["linpred_roofline"] = round(flop / (row["linpred_ms"] * 1e-3) / (MFMA_F32_TFLOPS * 1e12), 4) if row["linpred_ms"] > 0 else None
        print(json.dumps(row), flush=True)
        out.append(row)
        del flow, full, steps, th2
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
