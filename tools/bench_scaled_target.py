"""Reverse-KL training on the scaled-block GLM target (ScaledGLMTarget / AdditiveRegressionTarget, NF_TARGET_SCALEGLM), 65 536 draws:
per case one JSON line.
  gam       cfg-2 flow (RealNVP d = 64, hidden [64, 64], 8 couplings), a logit GAM with 1 024 rows: 4 linear columns and 4 smooth terms of
            14 basis columns under second-difference penalties with learned log-scales (p = 60, S = 4).  Arm a: the device target; arm b:
            the CLOSURE route (value_and_gradient with an ordinary torch `logp` doing the same arithmetic plus adam_update); arm c:
            MixedGLMTarget on the same rows at d = 64 with the scales frozen at 1 -- the same GEMM flop, so a's launch over c's is what
            the exp(-tau) path and the bins cost
  fullrank  a full-rank flow at d = 256 on the same model with 12 linear columns and 4 x 60 basis columns (arms a and b)
Per case: *_ms -- ms per training step of the arm (nf_elbo_step, asynchronous; the closure loop for arm b), *_launch_ms -- ms per
target launch ("target_scaleglm" / "target_mixglm": HIP events around the launch, nf_prof_read, in a run of its own) and *_roofline --
the launch's fraction of the fp32-MFMA figure on 4 R d N flop (two GEMMs, R the padded row count) over 157.3 TFLOP/s.  The arms' timed
loops alternate (a, b, c, a, ...) after a clock ramp of --ramp seconds; every figure is the median of --runs loops with the spread
(max - min) next to it.  The rows are also written to --out.
usage: python tools/bench_scaled_target.py [--runs 5] [--case gam,fullrank] [--out profiles/scaled_target.json]"""
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
from tools.bench_glm_targets import B1, B2, EPS, LR, MFMA_F32_TFLOPS, SIGMA, timed  # noqa: E402

N, ROWS, TERMS = 65536, 1024, 4
SCOPES = {"a": b"target_scaleglm", "c": b"target_mixglm"}


def gam(nf, px, m, gen):
    """(AdditiveRegressionTarget, the frozen-scale MixedGLMTarget at the same d, the closure) of one logit GAM"""
    p = px + TERMS * m
    A = (torch.randn(ROWS, p, generator=gen, dtype=torch.float64) / math.sqrt(p)).float().cuda()
    t = torch.randint(0, 2, (ROWS,), generator=gen).float().cuda()
    D2 = torch.diff(torch.eye(m, dtype=torch.float64), n=2, dim=0)
    pen = (D2.T @ D2).float().cuda()
    cols = [A[:, :px]] + [A[:, px + k * m:px + (k + 1) * m] for k in range(TERMS)]
    tgt = nf.AdditiveRegressionTarget("logit", cols[0], [(B, pen) for B in cols[1:]], t=t, prior_sigma=SIGMA)
    d = tgt.d
    wide = lambda M, at: torch.cat([torch.zeros(M.shape[0], at, device="cuda"), M, torch.zeros(M.shape[0], d - at - M.shape[1], device="cuda")], 1)  # noqa: E731
    sgn = (2.0 * t - 1.0)[:, None]
    frozen = nf.MixedGLMTarget([nf.GLMBlock("logit", wide(A * sgn, 0))] + [nf.GLMBlock("normal", wide(D2.float().cuda(), px + k * m)) for k in range(TERMS)],
                               prior_sigma=SIGMA)
    As, Dd = A * sgn, D2.float().cuda()

    def logp(ys):  # (d, N) -> (N,): the same density up to its constant
        beta, tau = ys[:p], ys[p:]
        lp = torch.nn.functional.logsigmoid(As @ beta).sum(0) - (beta * beta).sum(0) / (2 * SIGMA * SIGMA)
        for k in range(TERMS):
            r = Dd @ beta[px + k * m:px + (k + 1) * m]
            lp = lp - 0.5 * (r * r).sum(0) * torch.exp(-2.0 * tau[k]) - (m - 2) * tau[k]
        return lp - 0.5 * torch.exp(2.0 * tau).sum(0) + tau.sum(0)

    return tgt, frozen, logp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ramp", type=float, default=1.0)
    ap.add_argument("--case", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scaled_target.json"))
    args = ap.parse_args()
    nf = load_package()
    lib = nf.load_library()
    gen = torch.Generator().manual_seed(1)
    want = [c for c in args.case.split(",") if c]
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = []
    for case in ("gam", "fullrank"):
        if want and case not in want:
            continue
        if case == "fullrank":
            tgt, frozen, logp = gam(nf, 12, 60, gen)
            flow, fname = nf.fullrank(nf.MvNormal(tgt.d), paramtype=torch.float32), "fullrank_d256"
        else:
            tgt, frozen, logp = gam(nf, 4, 14, gen)
            flow, fname = nf.realnvp(nf.MvNormal(tgt.d), (64, 64), 4, paramtype=torch.float32, seed=1), "cfg2_realnvp_d64_h64x8"
        arms = {"a": tgt, "b": logp, "c": frozen}
        d = tgt.d
        theta0, re = flow.destructure()
        ctx = flow.ctx
        row = {"case": case, "flow": fname, "N": N, "d": d, "rows": tgt.rows, "blocks": tgt.rows // 32, "c_rows": frozen.rows}
        fns = {}
        for arm, tg in arms.items():
            th = theta0.clone()
            if arm == "b":  # the closure route
                st, rng = nf.setup(nf.Adam(LR), th), nf.PhiloxRNG(7)

                def fn(tg=tg, th=th, st=st, rng=rng):
                    _, g = nf.value_and_gradient(nf.elbo_batch, re(th), tg, N, rng)
                    nf.update(nf.Adam(LR), st, th, g, want_norm=True)
            else:
                m, v, k = torch.zeros_like(th), torch.zeros_like(th), [0]

                def fn(tg=tg, th=th, m=m, v=v, k=k):
                    nf._lib.check(lib.nf_elbo_step(ctx.ptr, C.byref(flow.desc), C.byref(tg.c), vp(th), vp(m), vp(v), N, 7, k[0], LR, B1, B2, EPS, None, None))
                    k[0] += 1
            fns[arm] = fn
            fn()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.ramp:  # clock ramp
            fns["a"]()
        torch.cuda.synchronize()
        ms = {arm: [] for arm in fns}
        for _ in range(args.runs):  # the arms alternate
            for arm, fn in fns.items():
                ms[arm].append(timed(fn))
        for arm, t in ms.items():
            row[arm + "_ms"], row[arm + "_spread"] = round(statistics.median(t), 4), round(max(t) - min(t), 4)
        row["b_over_a"] = round(row["b_ms"] / row["a_ms"], 3)
        per = {arm: [] for arm in SCOPES}  # the target launch alone, from events around it (runs of their own: the events perturb the step's timing)
        for _ in range(args.runs):
            for arm, scope in SCOPES.items():  # the arms alternate
                nf._lib.check(lib.nf_prof_enable(ctx.ptr, 2))
                for _ in range(20):
                    fns[arm]()
                t, cnt = C.c_double(0.0), C.c_int64(0)
                nf._lib.check(lib.nf_prof_read(ctx.ptr, scope, C.byref(t), C.byref(cnt)))
                nf._lib.check(lib.nf_prof_enable(ctx.ptr, 0))
                assert cnt.value == 20, (scope, cnt.value)
                per[arm].append(t.value)
        for arm, t in per.items():
            med = statistics.median(t)
            row[arm + "_launch_ms"], row[arm + "_launch_spread"] = round(med, 5), round(max(t) - min(t), 5)
            row[arm + "_roofline"] = round(4.0 * arms[arm].rows * d * N / (med * 1e-3) / (MFMA_F32_TFLOPS * 1e12), 4) if med > 0 else None
        row["a_over_c_launch"] = round(row["a_launch_ms"] / row["c_launch_ms"], 4)
        print(json.dumps(row), flush=True)
        out.append(row)
        del flow, fns, arms
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
