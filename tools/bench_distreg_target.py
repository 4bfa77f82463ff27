"""Reverse-KL training on the distributional regression targets (DistributionalRegressionTarget, NF_TARGET_DR_*), 65 536 draws, 1 024
rows: one JSON line per case.
  normal / student / zipoisson / weibull   cfg-2 flow (RealNVP d = 64, hidden [64, 64], 8 couplings), A = [X | Z] with p = q = 32:
                arm a  the kind itself,
                arm b  the CLOSURE route: value_and_gradient with an ordinary torch `logp` doing the same arithmetic plus adam_update --
                       how such a posterior is trained without the kind,
                arm c  GLMTarget("normal") on the same A: one predictor over all 64 columns, the same 4 R d N flop
  fullrank_d256 a full-rank flow at d = 256 (p = q = 128) on the Student family (arm a only)
Per case: x_ms -- ms per training step of the arm (nf_elbo_step, asynchronous; the closure loop for arm b), x_launch_ms -- ms per target
launch ("target_distreg" / "target_linpred": HIP events around the launch, nf_prof_read, in a run of its own) and x_roofline -- the
launch's fraction of the fp32-MFMA figure on 4 R d N flop (two GEMMs) over 157.3 TFLOP/s.  The arms' timed loops alternate (a, b, c,
a, ...) after a clock ramp of --ramp seconds; every figure is the median of --runs loops with the spread (max - min) next to it.
usage: python tools/bench_distreg_target.py [--runs 5] [--case normal,...,fullrank_d256] [--out profiles/distreg_target.json]"""
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

N, ROWS, NU = 65536, 1024, 4.0
FAMILIES = ("normal", "student", "zipoisson", "weibull")


def closure(family, X, Z, ou, ov, aux):
    """the torch form of the same posterior (flat constants left out: they do not change the arithmetic that is timed)"""
    a = aux[:, None]
    sp = torch.nn.functional.softplus

    def logp(ys):  # (d, N) -> (N,)
        p = X.shape[1]
        u, v = X @ ys[:p] + ou[:, None], Z @ ys[p:] + ov[:, None]
        if family in ("normal", "student"):
            z2 = (u * torch.exp(-v)) ** 2
            ph = (-0.5 * z2 if family == "normal" else -0.5 * (NU + 1.0) * torch.log1p(z2 / NU)) - v
        elif family == "zipoisson":
            m = torch.exp(u)
            ph = torch.where(a != 0, torch.logaddexp(v, -m), -m) - sp(v)
        else:
            w = u * torch.exp(v)
            ph = a * (v + w) - torch.exp(w)
        return ph.sum(0) - (ys * ys).sum(0) / (2 * SIGMA * SIGMA)

    return logp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ramp", type=float, default=1.0)
    ap.add_argument("--case", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distreg_target.json"))
    args = ap.parse_args()
    nf = load_package()
    lib = nf.load_library()
    gen = torch.Generator().manual_seed(1)
    want = [c for c in args.case.split(",") if c]
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = []
    for case in FAMILIES + ("fullrank_d256",):
        if want and case not in want:
            continue
        wide = case == "fullrank_d256"
        d, family = (256, "student") if wide else (64, case)
        p = d // 2
        A = (torch.randn(ROWS, d, generator=gen, dtype=torch.float64) / math.sqrt(d)).float().cuda()
        if family == "weibull":
            A[:, p:] *= 0.2  # (the shape exp(v) stays of order 1: exp(u exp(v)) is finite over the flow's draws)
        ou, ov = ((0.3 * torch.randn(ROWS, generator=gen, dtype=torch.float64)).float().cuda() for _ in range(2))
        aux = torch.randint(0, 2, (ROWS,), generator=gen).float().cuda()
        X, Z = A[:, :p].contiguous(), A[:, p:].contiguous()
        tgt = nf.DistributionalRegressionTarget(family, X, Z, ou, ov, None, aux, param=NU if family == "student" else 0.0, prior_sigma=SIGMA,
                                                prior_sigma_aux=SIGMA)
        if wide:
            flow, fname, arms = nf.fullrank(nf.MvNormal(d), paramtype=torch.float32), "fullrank_d256", {"a": tgt}
        else:
            flow, fname = nf.realnvp(nf.MvNormal(d), (64, 64), 4, paramtype=torch.float32, seed=1), "cfg2_realnvp_d64_h64x8"
            arms = {"a": tgt, "b": closure(family, X, Z, ou, ov, aux), "c": nf.GLMTarget("normal", A, ou, prior_sigma=SIGMA)}
        theta0, re = flow.destructure()
        ctx = flow.ctx
        row = {"case": case, "family": family, "flow": fname, "N": N, "d": d, "p": p, "rows": ROWS}
        fns, state = {}, {}
        for arm, t in arms.items():
            th = theta0.clone()
            if not hasattr(t, "c"):  # the closure route
                st, rng = nf.setup(nf.Adam(LR), th), nf.PhiloxRNG(7)

                def fn(t=t, th=th, st=st, rng=rng):
                    _, g = nf.value_and_gradient(nf.elbo_batch, re(th), t, N, rng)
                    nf.update(nf.Adam(LR), st, th, g, want_norm=True)
            else:
                m, v, k = torch.zeros_like(th), torch.zeros_like(th), [0]
                state[arm] = (th, m, v)

                def fn(t=t, th=th, m=m, v=v, k=k):
                    nf._lib.check(lib.nf_elbo_step(ctx.ptr, C.byref(flow.desc), C.byref(t.c), vp(th), vp(m), vp(v), N, 7, k[0], LR, B1, B2, EPS, None, None))
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
        for arm in ("b", "c"):
            if arm in ms:
                row[arm + "_over_a"] = round(row[arm + "_ms"] / row["a_ms"], 3)
        per = {arm: [] for arm in state}  # the target launch alone, from events around it (runs of their own: the events perturb the step's timing)
        for _ in range(args.runs):
            for arm in state:  # the arms alternate
                scope = b"target_distreg" if arm == "a" else b"target_linpred"
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
            row[arm + "_roofline"] = round(4.0 * ROWS * d * N / (med * 1e-3) / (MFMA_F32_TFLOPS * 1e12), 4) if med > 0 else None
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
