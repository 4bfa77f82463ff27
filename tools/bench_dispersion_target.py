"""Reverse-KL training on the GLM targets with a learned dispersion (DispersionGLMTarget: p = 55 coefficients, 48 of them in G = 8
groups with learned log-scales, the log-dispersion lambda, 1 024 data rows; normal and negbin families) with the cfg-2 flow (RealNVP
d = 64, hidden [64, 64], 8 couplings, 65 536 samples): per case one JSON line with
  step_ms / linpred_ms            -- ms per nf_elbo_step on the dispersion target and per "target_linpred" launch inside it (HIP events
                                     around the launch, nf_prof_read, in a run of its own),
  linpred_roofline                -- the launch's fraction of the fp32-MFMA roofline: 4 r d N flop (two GEMMs) over 157.3 TFLOP/s,
  hglm_step_ms / hglm_linpred_ms  -- the same flow and the same rows on the matching HierarchicalGLMTarget: sigma fixed (normal family)
                                     or the Poisson family (for negbin), a zero column standing where lambda sits: what the learned
                                     dispersion costs (per-lane exponentials, the counts' loads, the table loop),
  closure_ms                      -- ms per iteration of the CLOSURE route: value_and_gradient with an ordinary torch `logp` doing the
                                     same arithmetic plus adam_update -- how such a posterior is trained without the kinds,
  fullrank_step_ms                -- ms per nf_elbo_step of the full-rank Gaussian family on the same target,
and, for negbin, mt4096_linpred_ms: the launch with one count of 4097 (the longest table, 4096 entries).
The timed loops are interleaved after a clock ramp of --ramp seconds; every figure is the median of --runs loops, with the spread
(max - min) next to it.  --hglm-only times the HierarchicalGLMTarget launch alone; with --root it loads the package from another
checkout (a build of the parent commit), so that the two builds can be alternated on one box.
usage: python tools/bench_dispersion_target.py [--runs 5] [--case normal,negbin] [--out dispersion_target.json] [--hglm-only] [--root DIR]"""
import argparse
import ctypes as C
import importlib.util
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
MFMA_F32_TFLOPS = 157.3
SIGMA = 2.0
P, G, ROWS, N = 55, 8, 1024, 65536
HGLM_FAMILY = {"normal": "normal", "negbin": "poisson"}


def load_package(root):
    sys.path.insert(0, root)
    spec = importlib.util.spec_from_file_location("bench_graft_entry", os.path.join(root, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_package()


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


def make_data(gen):
    X = torch.randn(ROWS, P, generator=gen, dtype=torch.float64) / math.sqrt(P)
    off = 0.3 * torch.randn(ROWS, generator=gen, dtype=torch.float64)
    w = 0.5 + torch.rand(ROWS, generator=gen, dtype=torch.float64)
    k = torch.poisson(torch.full((ROWS,), 3.0, dtype=torch.float64), generator=gen)
    groups = torch.cat([torch.full((P - 6 * G,), -1), torch.arange(G).repeat_interleave(6)])  # 7 fixed-scale coefficients, 8 groups of 6
    hyper = ["halfcauchy", "halfnormal", "lognormal", "halfcauchy"] * 2
    return X, off, w, k, groups, hyper


def make_hglm(nf, family, data):
    """the matching hierarchical target at the flow's d = 64: the same rows, a zero column under N(0, 1) where lambda sits"""
    X, off, w, k, groups, hyper = data
    f = lambda t: t.float().cuda()
    gz = torch.cat([groups[:P - 6 * G], torch.tensor([-1]), groups[P - 6 * G:]])
    Xz = torch.cat([X[:, :P - 6 * G], torch.zeros(ROWS, 1, dtype=torch.float64), X[:, P - 6 * G:]], 1)
    return nf.HierarchicalGLMTarget(HGLM_FAMILY[family], f(Xz), gz.cuda(), G, f(off), f(w), fixed_sigma=SIGMA, hyper=hyper, hyper_scale=1.5)


def make_disp(nf, family, data, big_table=False):
    X, off, w, k, groups, hyper = data
    f = lambda t: t.float().cuda()
    if big_table:
        k = k.clone()
        k[0] = 4097.0
    return nf.DispersionGLMTarget(family, f(X), counts=f(k) if family == "negbin" else None, groups=groups.cuda(), n_groups=G, offset=f(off),
                                  weights=f(w), fixed_sigma=SIGMA, hyper=hyper, hyper_scale=1.5, disp_hyper="halfcauchy", disp_scale=1.5)


def make_closure(family, tgt, groups):
    """the torch closure of the dispersion density: the same buffers, torch arithmetic"""
    d = P + G + 1
    A, p0 = tgt.A, tgt.p0
    linv, offv, wtv = p0[:d], p0[d:d + ROWS], p0[d + ROWS:d + 2 * ROWS]
    at = d + 2 * ROWS
    c, mt = float(p0[at + 1]), int(p0[at + 2])
    at += 4 + P
    isd2 = (p0[at:at + P] ** 2)[:, None]
    at += P
    hm, his = p0[at:at + G + 1][:, None], p0[at + G + 1:at + 2 * G + 2][:, None]
    hk = [int(x) for x in p0[at + 2 * G + 2:at + 3 * G + 3].tolist()]
    at += 3 * (G + 1) + (G + 1) + P
    cnt, ctab = (p0[at:at + ROWS][:, None], p0[at + ROWS:at + ROWS + mt][:, None]) if family == "negbin" else (None, None)
    grouped = (groups >= 0).cuda()
    gi = groups.clamp(min=0).cuda()
    ms = torch.arange(1, mt + 1, dtype=torch.float32, device="cuda")[:, None]
    sp = torch.nn.functional.softplus

    def logp(ys):  # (d, N) -> (N,)
        beta, tl, lam = ys[:P], ys[P:], ys[d - 1]
        u = A @ ys + offv[:, None]
        om = torch.where(grouped[:, None], torch.exp(-2.0 * tl[gi]), isd2)
        x = tl - hm
        h = torch.stack([-0.5 * (x[g] * his[g]) ** 2 if hk[g] == 0 else -0.5 * torch.exp(2.0 * x[g]) if hk[g] == 1 else -sp(2.0 * x[g])
                         for g in range(G + 1)])
        if family == "negbin":
            rowsum = (wtv[:, None] * (-(cnt + torch.exp(lam)[None, :]) * sp(u - lam[None, :]))).sum(0) + (ctab * torch.log1p(ms * torch.exp(-lam)[None, :])).sum(0)
        else:
            rowsum = (wtv[:, None] * (-0.5 * (u * torch.exp(-lam)[None, :]) ** 2)).sum(0)
        return rowsum + linv @ ys - 0.5 * (beta * beta * om).sum(0) + h.sum(0) + c

    return logp


def linpred_ms(nf, lib, flow, step, iters=20):
    """ms per "target_linpred" launch from events around it (a run of its own: the events perturb the step's timing)"""
    nf._lib.check(lib.nf_prof_enable(flow.ctx.ptr, 2))
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    ms, cnt = C.c_double(0.0), C.c_int64(0)
    nf._lib.check(lib.nf_prof_read(flow.ctx.ptr, b"target_linpred", C.byref(ms), C.byref(cnt)))
    nf._lib.check(lib.nf_prof_enable(flow.ctx.ptr, 0))
    return round(ms.value, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ramp", type=float, default=1.0)
    ap.add_argument("--case", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--hglm-only", action="store_true")
    args = ap.parse_args()
    nf = load_package(os.path.abspath(args.root))
    lib = nf.load_library()
    d = P + G + 1
    want = [c for c in args.case.split(",") if c]
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = []
    for family in ("normal", "negbin"):
        if want and family not in want:
            continue
        data = make_data(torch.Generator().manual_seed(1))
        flow = nf.realnvp(nf.MvNormal(d), (64, 64), 4, paramtype=torch.float32, seed=1)
        flow = flow.with_theta(flow.theta * 0.3)  # the log-scales start within a few units
        hglm = make_hglm(nf, family, data)
        row = {"flow": "cfg2_realnvp_d64_h64x8", "target": f"disp_{family}_p{P}_G{G}_n{ROWS}", "N": N, "d": d, "rows": ROWS,
               "root": os.path.relpath(os.path.abspath(args.root), ROOT)}

        def stepper(fl, tgt):
            th = fl.theta.clone()
            m, v = torch.zeros_like(th), torch.zeros_like(th)
            k = [0]

            def step():
                nf._lib.check(lib.nf_elbo_step(fl.ctx.ptr, C.byref(fl.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), N, 7, k[0], LR, B1, B2, EPS, None, None))
                k[0] += 1

            return step

        if args.hglm_only:
            step = stepper(flow, hglm)
            step()
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < args.ramp:
                step()
            runs = [linpred_ms(nf, lib, flow, step) for _ in range(args.runs)]
            row["hglm_linpred_ms"], row["hglm_linpred_spread"] = statistics.median(runs), round(max(runs) - min(runs), 5)
            print(json.dumps(row), flush=True)
            out.append(row)
            continue
        full = nf.fullrank(nf.MvNormal(d), paramtype=torch.float32)
        disp = make_disp(nf, family, data)
        torch_logp = make_closure(family, disp, data[4])
        theta0, re = flow.destructure()
        steps = {"step": stepper(flow, disp), "hglm_step": stepper(flow, hglm), "fullrank_step": stepper(full, disp)}
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
        launches = {"linpred_ms": steps["step"], "hglm_linpred_ms": steps["hglm_step"]}
        if family == "negbin":
            big = make_disp(nf, family, data, big_table=True)
            row["mt4096_table_len"] = big.table_len
            launches["mt4096_linpred_ms"] = stepper(flow, big)
        for key, fn in launches.items():
            runs = [linpred_ms(nf, lib, flow, fn) for _ in range(args.runs)]
            row[key], row[key.replace("_ms", "_spread")] = statistics.median(runs), round(max(runs) - min(runs), 5)
        row["linpred_over_hglm"] = round(row["linpred_ms"] / row["hglm_linpred_ms"], 3)
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
