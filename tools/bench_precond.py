"""Preconditioned coupling flows (NF_KIND_PRECOND, y = mu + L T(x)) on the library's posterior targets, N = 65 536 draws, Float32:
the cfg-2 inner flow at d = 64 (RealNVP, hdims [64, 64], 8 couplings: LDS-resident, activation stash) and a weight-streaming
inner flow at d = 256 (hdims [256, 256], 4 couplings), on logistic regression with 1 024 rows and on a hierarchical logit model
(one varying intercept over 15 levels with a learned scale).  Per case one JSON row with
  precond_ms[arm]   -- ms per nf_elbo_step of the preconditioned flow in both arms of the full-rank layer's reverse pass: "fused"
                       (NF_PRECOND_BWD_SPLIT=0: k_fr_bwd_x) and "split" (NF_PRECOND_BWD_SPLIT=1: k_fr_bwd, then k_fr_gemm transposed),
  inner_ms, fullrank_ms -- ms per nf_elbo_step of the bare inner flow and of the bare full-rank family on the same target,
  fr_bwd_x_ms       -- the fused launch by HIP events, next to two_launch_ms = k_fr_bwd + the transposed k_fr_gemm it replaces
                       (the split arm's average k_fr_gemm launch is over the forward and the pullback: the pullback is twice that
                       average minus the fused arm's forward),
  loss_*            -- -ELBO on 16 384 fixed draws after --train-steps Adam steps (N = 4 096, lr 1e-3) of the bare inner flow, of
                       the full-rank family, and of the preconditioned flow started from the full-rank family at half the steps
                       and trained for the other half.
The switch is read once per process, so every arm runs in a child process of its own; the parent alternates the arms --rounds
times and reports the median with the spread (max - min).  The rows are also written to --out as one JSON list.
usage: python tools/bench_precond.py [--rounds 3] [--train-steps 200] [--dims 64,256] [--out profiles/precond.json]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
N, ROWS, LEVELS = 65536, 1024, 15
# d -> (hdims, blocks of two couplings).  64 and 256 are the workload; --dims 32,128 adds the two other tile geometries of the
# full-rank kernels (one and four 32-feature blocks), an LDS-resident and a weight-streaming inner flow
INNER = {32: ((32, 32), 4), 64: ((64, 64), 4), 128: ((128, 128), 2), 256: ((256, 256), 2)}


def make_target(nf, torch, name, d, gen):
    if name == "logreg":
        X = torch.randn(ROWS, d, generator=gen, dtype=torch.float64) / math.sqrt(d)
        t = torch.randint(0, 2, (ROWS,), generator=gen)
        return nf.LogisticRegressionTarget(X.float().cuda(), t.cuda(), prior_sigma=2.0)
    px = d - LEVELS - 1  # z = [b (px) ; one intercept per level ; the log-scale]
    X = torch.randn(ROWS, px, generator=gen, dtype=torch.float64) / math.sqrt(px)
    lev = torch.randint(0, LEVELS, (ROWS,), generator=gen)
    return nf.VaryingInterceptTarget("logit", X.float().cuda(), lev, LEVELS, fixed_sigma=2.0)


def timed(torch, fn, seconds=0.25, min_iters=5):
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


def child(args):
    import torch

    from __graft_entry__ import load_package

    nf = load_package()
    lib = nf.load_library()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    gen = torch.Generator().manual_seed(1)
    rows = []
    for d in args.dims:
        for tname in ("logreg", "hier_logit"):
            tgt = make_target(nf, torch, tname, d, gen)
            q0 = nf.MvNormal(d)
            hd, nl = INNER[d]
            flows = {"precond": nf.preconditioned(nf.realnvp(q0, hd, nl, paramtype=torch.float32))}
            if args.others:
                flows["inner"] = nf.realnvp(q0, hd, nl, paramtype=torch.float32)
                flows["fullrank"] = nf.fullrank(q0, paramtype=torch.float32)
            row = {"d": d, "target": tname, "N": N, "arm": args.child}
            steps = {}
            for key, flow in flows.items():
                th = flow.theta.clone()
                m, v = torch.zeros_like(th), torch.zeros_like(th)
                k = [0]

                def step(flow=flow, th=th, m=m, v=v, k=k):
                    nf._lib.check(lib.nf_elbo_step(flow.ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), N, 7, k[0], LR, B1, B2,
                                                   EPS, None, None))
                    k[0] += 1

                steps[key] = step
                step()
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < args.ramp:  # clock ramp
                steps["precond"]()
            torch.cuda.synchronize()
            ms = {key: [] for key in steps}
            for _ in range(args.runs):  # interleaved
                for key, step in steps.items():
                    ms[key].append(timed(torch, step))
            for key, vals in ms.items():
                row[key + "_ms"], row[key + "_spread"] = round(statistics.median(vals), 4), round(max(vals) - min(vals), 4)
            # the full-rank layer's launches alone, from events (a run of its own: the events perturb the step's timing)
            ctx = flows["precond"].ctx
            nf._lib.check(lib.nf_prof_enable(ctx.ptr, 2))
            for _ in range(20):
                steps["precond"]()
            torch.cuda.synchronize()
            for name in (b"fr_gemm", b"fr_bwd", b"fr_bwd_x"):
                a, cnt = C.c_double(0.0), C.c_int64(0)
                nf._lib.check(lib.nf_prof_read(ctx.ptr, name, C.byref(a), C.byref(cnt)))
                row[name.decode() + "_ms"], row[name.decode() + "_launches"] = round(a.value, 5), cnt.value // 20
            nf._lib.check(lib.nf_prof_enable(ctx.ptr, 0))
            if args.train_steps > 0:
                n_tr, half = 4096, args.train_steps // 2
                opt = nf.Adam(LR)

                def neg_elbo(flow):
                    return -nf.elbo_batch(nf.PhiloxRNG(99), flow, tgt, 16384)

                bare, _, _ = nf.train_flow(nf.elbo_batch, nf.realnvp(q0, hd, nl, paramtype=torch.float32), tgt, n_tr, max_iters=2 * half, optimiser=opt)
                fr_half, _, _ = nf.train_flow(nf.elbo_batch, nf.fullrank(q0, paramtype=torch.float32), tgt, n_tr, max_iters=half, optimiser=opt)
                fr_full, _, _ = nf.train_flow(nf.elbo_batch, nf.fullrank(q0, paramtype=torch.float32), tgt, n_tr, max_iters=2 * half, optimiser=opt)
                pre, _, _ = nf.train_flow(nf.elbo_batch, nf.preconditioned(nf.realnvp(q0, hd, nl, paramtype=torch.float32), init=fr_half), tgt, n_tr,
                                          max_iters=half, optimiser=opt)
                row.update(train_steps=2 * half, loss_inner=round(neg_elbo(bare), 4), loss_fullrank=round(neg_elbo(fr_full), 4),
                           loss_precond_from_fullrank=round(neg_elbo(pre), 4))
            rows.append(row)
            del flows, steps
            torch.cuda.empty_cache()
    print("ROWS " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ramp", type=float, default=1.0)
    ap.add_argument("--train-steps", type=int, default=200)
    ap.add_argument("--dims", type=lambda v: [int(x) for x in v.split(",")], default=[64, 256])
    ap.add_argument("--others", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child", choices=("fused", "split"), help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precond.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    per = {}
    for rnd in range(args.rounds):  # fused, split, fused, split, ...: the arms alternate on one box
        for arm in ("fused", "split"):
            env = dict(os.environ)
            env["NF_PRECOND_BWD_SPLIT"] = "1" if arm == "split" else "0"  # each arm forced, whatever the library would choose
            first = rnd == 0 and arm == "fused"  # the other flows and the training comparison: once
            cmd = [sys.executable, os.path.abspath(__file__), "--child", arm, "--runs", str(args.runs), "--ramp", str(args.ramp),
                   "--train-steps", str(args.train_steps if first else 0), "--dims", ",".join(map(str, args.dims))] + (["--others"] if first else [])
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-4000:])
                return p.returncode
            rows = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("ROWS ")][-1][5:])
            for r in rows:
                per.setdefault((r["d"], r["target"]), {}).setdefault(arm, []).append(r)
    out = []
    for (d, tname), arms in per.items():
        f0 = arms["fused"][0]
        row = {"flow": "preconditioned(realnvp)", "d": d, "target": tname, "N": N, "inner_hdims": list(INNER[d][0]), "couplings": 2 * INNER[d][1]}
        for arm in ("fused", "split"):
            vals = [r["precond_ms"] for r in arms[arm]]
            row[f"precond_ms_{arm}"], row[f"precond_spread_{arm}"] = round(statistics.median(vals), 4), round(max(vals) - min(vals), 4)
            row[f"precond_ms_{arm}_rounds"] = vals
        for key in ("inner_ms", "inner_spread", "fullrank_ms", "fullrank_spread", "train_steps", "loss_inner", "loss_fullrank",
                    "loss_precond_from_fullrank"):
            if key in f0:
                row[key] = f0[key]
        fx = [r["fr_bwd_x_ms"] for r in arms["fused"]]
        fwd = statistics.median(r["fr_gemm_ms"] for r in arms["fused"])
        two = [r["fr_bwd_ms"] + 2.0 * r["fr_gemm_ms"] - fwd for r in arms["split"]]
        row["fr_bwd_x_ms"], row["fr_bwd_x_spread"] = round(statistics.median(fx), 5), round(max(fx) - min(fx), 5)
        row["two_launch_ms"], row["two_launch_spread"] = round(statistics.median(two), 5), round(max(two) - min(two), 5)
        row["fr_gemm_forward_ms"] = round(fwd, 5)
        print(json.dumps(row), flush=True)
        out.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
