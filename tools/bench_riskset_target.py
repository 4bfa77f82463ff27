"""Reverse-KL training on the risk-set regression target (RiskSetTarget through its two wrappers, 1 024 data rows, 65 536 samples):
  flows   cfg2      the cfg-2 flow (RealNVP d = 64, hidden [64, 64], 8 couplings), p = 64 features,
          fullrank  the full-rank Gaussian family at d = 256, p = 256 features;
  data    cox       CoxRegressionTarget, one stratum, distinct times, about 60 % events: ONE segment of 1 024 rows,
          clogit    ConditionalLogitTarget with choice sets of 4: 256 segments.
Per case one JSON line with
  riskset_ms        -- ms per "target_riskset" launch (HIP events around the launch, nf_prof_read) inside nf_elbo_step,
  riskset_roofline  -- its fraction of the fp32-MFMA figure on 6 R p N flop (GEMM 1 twice -- the recompute -- and GEMM 2, over the
                       R padded rows) over 157.3 TFLOP/s,
  step_ms           -- ms per nf_elbo_step with the built-in target (asynchronous: no host read),
  glm_step_ms       -- ms per nf_elbo_step of the SAME flow on GLMTarget("logit") over the same rows (A = X): the yardstick, one GEMM
                       pair and one log-sigmoid per element; glm_ms is its "target_linpred" launch,
  closure_ms        -- ms per iteration of the CLOSURE route on the same box and in the same process: value_and_gradient with an
                       ordinary torch `logp` doing the same arithmetic (matmul, torch.logcumsumexp inside the segments, the masses
                       gathered; library forward that keeps its tape, torch autograd for the score, library pullback) plus
                       adam_update -- how such a posterior is trained without the kind.
The timed loops are interleaved (step, glm, closure, step, ...) after a clock ramp of --ramp seconds; every figure is the median of
--runs loops, with the spread (max - min) next to it.  The rows are also written to --out as one JSON list.
usage: python tools/bench_riskset_target.py [--runs 5] [--case cfg2_cox,fullrank_clogit] [--out profiles/riskset_target.json]"""
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


def torch_form(tgt, seglen):
    """the torch closure of the target from its own device buffers (segments of one length, no padding): matmul, logcumsumexp, gather"""
    R, p = tgt.padded_rows, tgt.p
    assert R == tgt.rows and R % seglen == 0
    X, off, lw, m = tgt.A, tgt.p0[:R], tgt.p0[R:2 * R], tgt.p0[2 * R:3 * R]
    lin, prec, c0 = tgt.p0[4 * R:4 * R + p], float(tgt.p0[4 * R + p]), float(tgt.p0[4 * R + p + 1])
    shift = (off + lw)[:, None]
    rows = torch.nonzero(m > 0)[:, 0]
    mk = m[rows][:, None]

    def logp(ys):  # (d, N) -> (N,)
        a = X @ ys + shift                                                  # [R, N]
        c = torch.logcumsumexp(a.view(R // seglen, seglen, -1), 1).view(R, -1)
        return c0 + lin @ ys - (mk * c[rows]).sum(0) - 0.5 * prec * (ys * ys).sum(0)

    return logp


def make_targets(nf, data, p, rows, gen):
    X = torch.randn(rows, p, generator=gen, dtype=torch.float64) / math.sqrt(p)
    if data == "cox":
        time_ = torch.randperm(rows, generator=gen).double()
        event = (torch.rand(rows, generator=gen) < 0.6).double()
        tgt, seglen = nf.CoxRegressionTarget(X.float().cuda(), time_, event, prior_sigma=SIGMA), rows
    else:
        cs = torch.arange(rows) // 4
        chosen = torch.zeros(rows)
        chosen[4 * torch.arange(rows // 4) + torch.randint(0, 4, (rows // 4,), generator=gen)] = 1.0
        tgt, seglen = nf.ConditionalLogitTarget(X.float().cuda(), cs, chosen, prior_sigma=SIGMA), 4
    glm = nf.GLMTarget("logit", tgt.A, prior_sigma=SIGMA)
    return tgt, torch_form(tgt, seglen), glm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ramp", type=float, default=1.0)
    ap.add_argument("--case", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "riskset_target.json"))
    args = ap.parse_args()
    nf = load_package()
    lib = nf.load_library()
    gen = torch.Generator().manual_seed(1)
    rows, n = 1024, 65536
    flows = [("cfg2", "cfg2_realnvp_d64_h64x8", 64, lambda d: nf.realnvp(nf.MvNormal(d), (64, 64), 4, paramtype=torch.float32, seed=1)),
             ("fullrank", "fullrank_d256", 256, lambda d: nf.fullrank(nf.MvNormal(d), paramtype=torch.float32))]
    want = [c for c in args.case.split(",") if c]
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = []
    for cname, fname, d, make_flow in flows:
        for data in ("cox", "clogit"):
            if want and f"{cname}_{data}" not in want:
                continue
            flow = make_flow(d)
            tgt, torch_logp, glm = make_targets(nf, data, d, rows, gen)
            theta0, re = flow.destructure()
            row = {"flow": fname, "target": f"riskset_{data}_p{d}_n{rows}", "N": n, "d": d, "rows": rows, "padded_rows": tgt.padded_rows,
                   "segments": int(tgt.segment_start.sum())}
            ctx = flow.ctx
            # the closure and the kind compute the same density (a few points, before anything is timed)
            ys = 0.5 * torch.randn(d, 8, device="cuda")
            dev_lp = nf.target_logp(tgt, ys)
            row["closure_vs_kind_max_rel"] = float(((torch_logp(ys) - dev_lp).abs() / dev_lp.abs()).max())

            def stepper(target):
                th = theta0.clone()
                m, v = torch.zeros_like(th), torch.zeros_like(th)
                k = [0]

                def step():
                    nf._lib.check(lib.nf_elbo_step(ctx.ptr, C.byref(flow.desc), C.byref(target.c), vp(th), vp(m), vp(v), n, 7, k[0], LR, B1, B2, EPS, None, None))
                    k[0] += 1

                return step, (th, m, v)

            step, keep_a = stepper(tgt)
            glm_step, keep_b = stepper(glm)
            th2 = theta0.clone()
            st = nf.setup(nf.Adam(LR), th2)
            rng = nf.PhiloxRNG(7)

            def closure():
                _, g = nf.value_and_gradient(nf.elbo_batch, re(th2), torch_logp, n, rng)
                nf.update(nf.Adam(LR), st, th2, g, want_norm=True)

            step()
            glm_step()
            closure()
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < args.ramp:  # clock ramp
                step()
            torch.cuda.synchronize()
            a, b, c = [], [], []
            for _ in range(args.runs):  # interleaved
                a.append(timed(step))
                b.append(timed(glm_step))
                c.append(timed(closure))
            row["step_ms"], row["step_spread"] = round(statistics.median(a), 4), round(max(a) - min(a), 4)
            row["glm_step_ms"], row["glm_step_spread"] = round(statistics.median(b), 4), round(max(b) - min(b), 4)
            row["closure_ms"], row["closure_spread"] = round(statistics.median(c), 4), round(max(c) - min(c), 4)
            row["closure_over_step"] = round(row["closure_ms"] / row["step_ms"], 3)
            row["step_over_glm_step"] = round(row["step_ms"] / row["glm_step_ms"], 3)
            # the target launches alone, from events around them (runs of their own: the events perturb the step's timing)
            for fn, scope, key in ((step, b"target_riskset", "riskset"), (glm_step, b"target_linpred", "glm")):
                nf._lib.check(lib.nf_prof_enable(ctx.ptr, 2))
                for _ in range(20):
                    fn()
                torch.cuda.synchronize()
                ms, cnt = C.c_double(0.0), C.c_int64(0)
                nf._lib.check(lib.nf_prof_read(ctx.ptr, scope, C.byref(ms), C.byref(cnt)))
                nf._lib.check(lib.nf_prof_enable(ctx.ptr, 0))
                row[key + "_ms"], row[key + "_launches"] = round(ms.value, 5), cnt.value
            row["riskset_over_glm_launch"] = round(row["riskset_ms"] / row["glm_ms"], 3) if row["glm_ms"] > 0 else None
            flop = 6.0 * tgt.padded_rows * d * n
            row["riskset_gflop"] = round(flop / 1e9, 3)
            row["riskset_roofline"] = round(flop / (row["riskset_ms"] * 1e-3) / (MFMA_F32_TFLOPS * 1e12), 4) if row["riskset_ms"] > 0 else None
            print(json.dumps(row), flush=True)
            out.append(row)
            del flow, keep_a, keep_b, th2, tgt, glm, torch_logp
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
