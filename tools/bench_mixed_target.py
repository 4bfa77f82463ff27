"""Reverse-KL training on the mixed-family GLM target (MixedGLMTarget, NF_TARGET_MIXGLM), 65 536 draws: per case one JSON line.
  dispatch      cfg-2 flow (RealNVP d = 64, hidden [64, 64], 8 couplings), logistic regression with 1 024 rows: MixedGLMTarget of
                the likelihood alone (arm a) against GLMTarget("logit") on the same rows (arm b) -- what the per-block dispatch costs
  cauchy_prior  the same flow and likelihood plus 64 Cauchy prior rows (arm a) against the CLOSURE route (arm b): value_and_gradient
                with an ordinary torch `logp` doing the same arithmetic plus adam_update -- how such a posterior is trained without
                the kind
  six_families  a full-rank flow at d = 256 on a six-family target of 1 216 rows (arm a only)
Per case: a_ms / b_ms -- ms per training step of the arm (nf_elbo_step, asynchronous; the closure loop for cauchy_prior's arm b),
a_launch_ms / b_launch_ms -- ms per target launch ("target_mixglm" / "target_linpred": HIP events around the launch, nf_prof_read, in
a run of its own) and a_roofline / b_roofline -- the launch's fraction of the fp32-MFMA figure on 4 R d N flop (two GEMMs, R the
padded row count) over 157.3 TFLOP/s.  The two arms' timed loops alternate (a, b, a, b, ...) after a clock ramp of --ramp seconds;
every figure is the median of --runs loops with the spread (max - min) next to it.  The rows are also written to --out.
usage: python tools/bench_mixed_target.py [--runs 5] [--case dispatch,cauchy_prior,six_families] [--out profiles/mixed_target.json]"""
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

N = 65536


def logit_rows(d, rows, gen):
    X = torch.randn(rows, d, generator=gen, dtype=torch.float64) / math.sqrt(d)
    sign = 2.0 * torch.randint(0, 2, (rows,), generator=gen).double() - 1.0
    return (X * sign[:, None]).float().cuda()


def cauchy_closure(A, d):
    """the torch form of logistic likelihood + N(0, SIGMA^2 I) + independent Cauchy(0, 1) priors on every coefficient"""
    c = -0.5 * d * math.log(2 * math.pi * SIGMA * SIGMA) - d * math.log(math.pi)

    def logp(ys):  # (d, N) -> (N,)
        return torch.nn.functional.logsigmoid(A @ ys).sum(0) - torch.log1p(ys * ys).sum(0) - (ys * ys).sum(0) / (2 * SIGMA * SIGMA) + c

    return logp


def six_families(nf, d, gen):
    rnd = lambda r: (torch.randn(r, d, generator=gen, dtype=torch.float64) / math.sqrt(d)).float().cuda()  # noqa: E731
    off = lambda r: (0.3 * torch.randn(r, generator=gen, dtype=torch.float64)).float().cuda()  # noqa: E731
    like = torch.zeros(1, device="cuda")
    S = torch.diff(torch.eye(d, dtype=torch.float64), dim=0)
    return nf.MixedGLMTarget([nf.GLMBlock("logit", rnd(512)), nf.GLMBlock("probit", rnd(128), off(128)), nf.GLMBlock("poisson", rnd(128), off(128)),
                              nf.GLMBlock("student", rnd(128), off(128), param=4.0), nf.gaussian_penalty(S.T @ S, like),
                              nf.coefficient_prior("check", d, like, index=list(range(64)))], prior_sigma=SIGMA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ramp", type=float, default=1.0)
    ap.add_argument("--case", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_target.json"))
    args = ap.parse_args()
    nf = load_package()
    lib = nf.load_library()
    gen = torch.Generator().manual_seed(1)
    want = [c for c in args.case.split(",") if c]
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = []
    for case in ("dispatch", "cauchy_prior", "six_families"):
        if want and case not in want:
            continue
        d = 256 if case == "six_families" else 64
        if case == "six_families":
            flow, fname = nf.fullrank(nf.MvNormal(d), paramtype=torch.float32), "fullrank_d256"
            arms = {"a": six_families(nf, d, gen)}
        else:
            flow, fname = nf.realnvp(nf.MvNormal(d), (64, 64), 4, paramtype=torch.float32, seed=1), "cfg2_realnvp_d64_h64x8"
            A = logit_rows(d, 1024, gen)
            glm = nf.GLMTarget("logit", A, prior_sigma=SIGMA)
            if case == "dispatch":
                arms = {"a": nf.MixedGLMTarget([glm]), "b": glm}
            else:
                arms = {"a": nf.MixedGLMTarget([glm, nf.coefficient_prior("student", d, A, param=1.0)]), "b": cauchy_closure(A, d)}
        theta0, re = flow.destructure()
        ctx = flow.ctx
        row = {"case": case, "flow": fname, "N": N, "d": d, "rows": arms["a"].rows, "blocks": arms["a"].rows // 32}
        fns, state = {}, {}
        for arm, tgt in arms.items():
            th = theta0.clone()
            if callable(tgt) and not hasattr(tgt, "c"):  # the closure route
                st, rng = nf.setup(nf.Adam(LR), th), nf.PhiloxRNG(7)

                def fn(tgt=tgt, th=th, st=st, rng=rng):
                    _, g = nf.value_and_gradient(nf.elbo_batch, re(th), tgt, N, rng)
                    nf.update(nf.Adam(LR), st, th, g, want_norm=True)
            else:
                m, v, k = torch.zeros_like(th), torch.zeros_like(th), [0]
                state[arm] = (th, m, v)

                def fn(tgt=tgt, th=th, m=m, v=v, k=k):
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
            for arm, fn in fns.items():
                ms[arm].append(timed(fn))
        for arm, t in ms.items():
            row[arm + "_ms"], row[arm + "_spread"] = round(statistics.median(t), 4), round(max(t) - min(t), 4)
        if "b" in ms:
            row["b_over_a"] = round(row["b_ms"] / row["a_ms"], 3)
        per = {arm: [] for arm in state}  # the target launch alone, from events around it (runs of their own: the events perturb the step's timing)
        for _ in range(args.runs):
            for arm in state:  # the arms alternate
                scope = b"target_mixglm" if arm == "a" else b"target_linpred"
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
        print(json.dumps(row), flush=True)
        out.append(row)
        del flow, fns, state, arms
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
