"""Reverse-KL training on the correlated-random-effects targets (CorrelatedEffectsTarget, "dnormal": lmer(y ~ x + (x | g)) with a learned
residual scale), 65 536 draws, 1 024 rows; per case one JSON line with
  step_ms / correff_ms        -- ms per nf_elbo_step and per "target_correff" launch inside it (HIP events around the launch, nf_prof_read,
                                 in a run of its own),
  indep_step_ms / indep_ms    -- the same flow on a DispersionGLMTarget over the same rows with every effect under an INDEPENDENT learned
                                 scale ((1 + x || g)), padded with zero columns to the same d: the same GEMM flop, so
  epilogue_ratio              -- correff_ms / indep_ms is the price of the correlated prior's epilogue,
  closure_ms                  -- ms per iteration of the closure route: value_and_gradient with a torch `logp` doing the same arithmetic
                                 (library forward that keeps its tape, torch autograd for the score, library pullback) plus adam_update.
Cases: "cfg2" -- RealNVP, hidden [64, 64], 8 couplings on the sleepstudy shape (p = 2, one term k = 2, G = 28: d = 62);
"fullrank" -- the full-rank Gaussian family on k = 4, G = 60, p = 5: d = 256.  The timed loops alternate (correff, indep, closure,
correff, ...) after a clock ramp; every figure is the median of --runs loops with the spread (max - min) next to it.
usage: python tools/bench_correff_target.py [--runs 5] [--case cfg2,fullrank] [--out profiles/correff_target.json]"""
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
from bench_hier_target import B1, B2, EPS, LR, timed  # noqa: E402

ROWS, N = 1024, 65536
CASES = {"cfg2": (2, 2, 28), "fullrank": (5, 4, 60)}  # p, k, G


def make_targets(nf, p, k, G, gen):
    """the correlated target, the independent-scales target over the same rows at the same d, and the torch closure of the former"""
    X = torch.randn(ROWS, p, generator=gen, dtype=torch.float64) / math.sqrt(p)
    Z = torch.cat([torch.ones(ROWS, 1, dtype=torch.float64), torch.randn(ROWS, k - 1, generator=gen, dtype=torch.float64)], 1)
    lev = torch.randint(0, G, (ROWS,), generator=gen)
    t = torch.randn(ROWS, generator=gen, dtype=torch.float64)
    f = lambda v: v.float().cuda()
    cre = nf.MixedEffectsRegressionTarget("dnormal", f(X), [(f(Z), lev.cuda(), G, 2.0)], t=f(t), fixed_sigma=2.0, hyper="halfnormal", hyper_scale=1.5, disp_hyper="halfnormal")
    d, m = cre.d, k * (k - 1) // 2
    pa = p + G * k
    cols = torch.cat([torch.arange(pa), torch.arange(pa + k, pa + k + m)])  # beta, b and omega's (zero) columns: p + G k + m coefficients
    groups = torch.cat([torch.full((p,), -1), torch.arange(k).repeat(G), torch.full((m,), -1)])
    ind = nf.DispersionGLMTarget("normal", cre.A[:, cols].contiguous(), None, groups.cuda(), k, cre.p0[d:d + ROWS].clone(), None, None,
                                 -0.5 * math.log(2.0 * math.pi) * ROWS, fixed_sigma=2.0, hyper="halfnormal", hyper_scale=1.5)
    assert ind.d == d
    A, p0 = cre.A, cre.p0
    lin, off, wt, c = p0[:d], p0[d:d + ROWS], p0[d + ROWS:d + 2 * ROWS], float(p0[d + 2 * ROWS + 1])
    fom = p0[d + 2 * ROWS + 4:2 * d + 2 * ROWS + 4]
    tab = p0[2 * d + 2 * ROWS + 4:2 * d + 2 * ROWS + 28].tolist()
    ib, it, io = int(tab[2]), int(tab[3]), int(tab[4])
    lamh = p0[-4:].tolist()
    hm = math.log(1.5)

    def logp(ys):  # (d, N) -> (N,): the packed layout's arithmetic in plain torch
        lam, tau, z = ys[-1], ys[it:io], torch.tanh(ys[io:io + m])
        u = (A @ ys + off[:, None]) * torch.exp(-lam)
        out = c + (wt[:, None] * (-0.5 * u * u)).sum(0) + lin @ ys - 0.5 * (fom[:, None] * ys * ys).sum(0) - 0.5 * torch.exp(2.0 * (lam - lamh[1]))
        a = torch.exp(-tau)[None] * ys[ib:it].reshape(G, k, -1)
        zz, n = [], 0
        for i in range(k):
            rem, acc = torch.ones_like(lam), a[:, i]
            for j in range(i):
                lij = z[n] * torch.sqrt(rem)
                out = out + tab[5 + n] * torch.log1p(-z[n] * z[n])
                acc, rem, n = acc - lij * zz[j], rem - lij * lij, n + 1
            zz.append(acc / torch.sqrt(rem))
            out = out - 0.5 * (zz[i] * zz[i]).sum(0) - G * (tau[i] + 0.5 * torch.log(rem)) - 0.5 * torch.exp(2.0 * (tau[i] - hm))
        return out

    return cre, ind, logp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ramp", type=float, default=1.0)
    ap.add_argument("--case", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correff_target.json"))
    args = ap.parse_args()
    nf = load_package()
    lib = nf.load_library()
    gen = torch.Generator().manual_seed(1)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = []
    for name, (p, k, G) in CASES.items():
        if args.case and name not in args.case.split(","):
            continue
        cre, ind, torch_logp = make_targets(nf, p, k, G, gen)
        d = cre.d
        ys = 0.5 * torch.randn(d, 64, generator=gen).cuda()  # the closure is the library's density
        assert torch.allclose(torch_logp(ys), nf.target_logp(cre, ys), rtol=1e-3, atol=1e-2)
        if name == "cfg2":
            flow = nf.realnvp(nf.MvNormal(d), (64, 64), 4, paramtype=torch.float32, seed=1)
            flow = flow.with_theta(flow.theta * 0.3)  # the log-scales start within a few units
        else:
            flow = nf.fullrank(nf.MvNormal(d), paramtype=torch.float32)
        theta0, re = flow.destructure()
        row = {"case": name, "target": f"correff_dnormal_p{p}_k{k}_G{G}_n{ROWS}", "N": N, "d": d, "rows": ROWS}

        def stepper(tgt):
            th = flow.theta.clone()
            mm, v = torch.zeros_like(th), torch.zeros_like(th)
            it = [0]

            def step():
                nf._lib.check(lib.nf_elbo_step(flow.ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(mm), vp(v), N, 7, it[0], LR, B1, B2, EPS, None, None))
                it[0] += 1

            return step

        steps = {"step": stepper(cre), "indep_step": stepper(ind)}
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
        times = {key: [] for key in steps}
        for _ in range(args.runs):  # alternating
            for key, fn in steps.items():
                times[key].append(timed(fn))
        for key, v in times.items():
            row[key + "_ms"], row[key + "_spread"] = round(statistics.median(v), 4), round(max(v) - min(v), 4)
        row["closure_over_step"] = round(row["closure_ms"] / row["step_ms"], 3)
        for key, sname, scope in (("correff_ms", "step", b"target_correff"), ("indep_ms", "indep_step", b"target_linpred")):
            nf._lib.check(lib.nf_prof_enable(flow.ctx.ptr, 2))  # runs of their own: the events perturb the step's timing
            for _ in range(20):
                steps[sname]()
            torch.cuda.synchronize()
            ms, cnt = C.c_double(0.0), C.c_int64(0)
            nf._lib.check(lib.nf_prof_read(flow.ctx.ptr, scope, C.byref(ms), C.byref(cnt)))
            nf._lib.check(lib.nf_prof_enable(flow.ctx.ptr, 0))
            row[key] = round(ms.value, 5)
        row["epilogue_ratio"] = round(row["correff_ms"] / row["indep_ms"], 3) if row["indep_ms"] > 0 else None
        print(json.dumps(row), flush=True)
        out.append(row)
        del flow, steps, th2
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
