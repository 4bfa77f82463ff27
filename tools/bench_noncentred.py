"""Non-centred flows (NF_KIND_NONCENTRED, y = S(T(x))) on the hierarchical logit target of tools/bench_precond.py (one varying
intercept over 15 levels with a learned scale, 1 024 rows), N = 65 536 draws, Float32.  Inner flows: the cfg-2 RealNVP at d = 64
(hdims [64, 64], 8 couplings: LDS-resident, activation stash), a weight-streaming RealNVP at d = 256 (hdims [256, 256], 4
couplings) and the full-rank family at both.  Per case one JSON row with
  noncentred_ms, inner_ms -- ms per nf_elbo_step of the non-centred flow and of its bare inner flow: each arm in child processes of
                             its own, the parent alternates them --rounds times and reports the median with the spread (max - min),
  nc_fwd_ms, nc_bwd_ms    -- the layer's two launches by HIP events (a run of its own), and the fraction of the HBM copy figure of
                             DESIGN section 4 (4.7 TB/s) they reach: the forward moves 2 d N floats, the reverse launch 3 d N.
--fit adds the table the kind exists for: -ELBO on 16 384 fixed draws after --train-steps Adam steps (4 096 draws, lr 1e-3) of the
bare RealNVP, the bare full-rank family, noncentred(realnvp) and noncentred(fullrank) from lam = 1 (trained; the latter frozen
too) and noncentred(realnvp) from lam = 0.  The rows are also written to --out as one JSON object.
usage: python tools/bench_noncentred.py [--rounds 3] [--fit] [--train-steps 200] [--out profiles/noncentred.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_precond import B1, B2, EPS, INNER, LR, N, make_target, timed  # noqa: E402

HBM_COPY = 4.7e12  # bytes / s
CASES = [(64, "realnvp"), (64, "fullrank"), (256, "realnvp"), (256, "fullrank")]


def hier_targets(nf, torch):
    """d -> the hierarchical logit target of tools/bench_precond.py at 64 and 256: its generator, walked in its order"""
    gen, out = torch.Generator().manual_seed(1), {}
    for d in (64, 256):
        make_target(nf, torch, "logreg", d, gen)
        out[d] = make_target(nf, torch, "hier_logit", d, gen)
    return out


def make_inner(nf, torch, d, kind):
    q0 = nf.MvNormal(d)
    if kind == "fullrank":
        return nf.fullrank(q0, paramtype=torch.float32)
    hd, nl = INNER[d]
    return nf.realnvp(q0, hd, nl, paramtype=torch.float32)


def child(args):
    import torch

    from __graft_entry__ import load_package

    nf = load_package()
    lib = nf.load_library()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rows, targets = [], hier_targets(nf, torch)
    for d, kind in CASES:
        tgt = targets[d]
        inner = make_inner(nf, torch, d, kind)
        flow = nf.noncentred(inner, tgt) if args.child == "noncentred" else inner
        th = flow.theta.clone()
        m, v = torch.zeros_like(th), torch.zeros_like(th)
        k = [0]

        def step():
            nf._lib.check(lib.nf_elbo_step(flow.ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), N, 7, k[0], LR, B1, B2, EPS,
                                           None, None))
            k[0] += 1

        step()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.ramp:  # clock ramp
            step()
        torch.cuda.synchronize()
        vals = [timed(torch, step) for _ in range(args.runs)]
        row = {"d": d, "inner": kind, "arm": args.child, "ms": round(statistics.median(vals), 4)}
        if args.child == "noncentred":  # the layer's launches alone, from events (a run of its own: the events perturb the step's timing)
            ctx = flow.ctx
            nf._lib.check(lib.nf_prof_enable(ctx.ptr, 2))
            for _ in range(20):
                step()
            torch.cuda.synchronize()
            for name in (b"nc_fwd", b"nc_bwd"):
                a, cnt = C.c_double(0.0), C.c_int64(0)
                nf._lib.check(lib.nf_prof_read(ctx.ptr, name, C.byref(a), C.byref(cnt)))
                row[name.decode() + "_ms"], row[name.decode() + "_launches"] = round(a.value, 5), cnt.value // 20
            nf._lib.check(lib.nf_prof_enable(ctx.ptr, 0))
        rows.append(row)
        del flow, inner
        torch.cuda.empty_cache()
    print("ROWS " + json.dumps(rows), flush=True)


def fit(args):
    import torch

    from __graft_entry__ import load_package

    nf = load_package()
    rows, targets = [], hier_targets(nf, torch)
    for d in (64, 256):
        tgt = targets[d]
        arms = {
            "realnvp": lambda: make_inner(nf, torch, d, "realnvp"),
            "fullrank": lambda: make_inner(nf, torch, d, "fullrank"),
            "noncentred(realnvp) lam=1": lambda: nf.noncentred(make_inner(nf, torch, d, "realnvp"), tgt),
            "noncentred(fullrank) lam=1": lambda: nf.noncentred(make_inner(nf, torch, d, "fullrank"), tgt),
            "noncentred(fullrank) lam=1 frozen": lambda: nf.noncentred(make_inner(nf, torch, d, "fullrank"), tgt, learn=False),
            "noncentred(realnvp) lam=0": lambda: nf.noncentred(make_inner(nf, torch, d, "realnvp"), tgt, lam=0.0),
        }
        row = {"d": d, "target": "hier_logit", "train_steps": args.train_steps, "draws": 4096, "lr": LR}
        for name, make in arms.items():
            trained, _, _ = nf.train_flow(nf.elbo_batch, make(), tgt, 4096, max_iters=args.train_steps, optimiser=nf.Adam(LR))
            row[name] = round(-nf.elbo_batch(nf.PhiloxRNG(99), trained, tgt, 16384), 4)
            if trained.kind == "noncentred":  # the learned lam of the coefficients that have a group (the 15 intercepts)
                lam = trained.lam[torch.tensor((tgt.groups >= 0).numpy(), device=trained.lam.device)]
                row[name + " lam"] = [round(float(lam.min()), 4), round(float(lam.mean()), 4), round(float(lam.max()), 4)]
        rows.append(row)
    print("ROWS " + json.dumps(rows), flush=True)


def run_child(args, extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--runs", str(args.runs), "--ramp", str(args.ramp), "--train-steps", str(args.train_steps)] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        return None
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("ROWS ")][-1][5:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ramp", type=float, default=1.0)
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--train-steps", type=int, default=200)
    ap.add_argument("--child", choices=("noncentred", "inner", "fit"), help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noncentred.json"))
    args = ap.parse_args()
    if args.child == "fit":
        return fit(args)
    if args.child:
        return child(args)
    per = {}
    for _ in range(args.rounds):  # noncentred, inner, noncentred, inner, ...: the arms alternate on one box
        for arm in ("noncentred", "inner"):
            rows = run_child(args, ["--child", arm])
            if rows is None:
                return 1
            for r in rows:
                per.setdefault((r["d"], r["inner"]), {}).setdefault(arm, []).append(r)
    steps = []
    for (d, kind), arms in per.items():
        row = {"flow": f"noncentred({kind})", "d": d, "target": "hier_logit", "N": N}
        if kind == "realnvp":
            row.update(inner_hdims=list(INNER[d][0]), couplings=2 * INNER[d][1])
        for arm in ("noncentred", "inner"):
            vals = [r["ms"] for r in arms[arm]]
            row[f"{arm}_ms"], row[f"{arm}_spread"], row[f"{arm}_ms_rounds"] = round(statistics.median(vals), 4), round(max(vals) - min(vals), 4), vals
        for name, floats in (("nc_fwd", 2), ("nc_bwd", 3)):
            vals = [r[name + "_ms"] for r in arms["noncentred"]]
            ms = statistics.median(vals)
            row[name + "_ms"], row[name + "_spread"] = round(ms, 5), round(max(vals) - min(vals), 5)
            row[name + "_launches_per_step"] = arms["noncentred"][0][name + "_launches"]
            row[name + "_hbm_copy_fraction"] = round(floats * d * N * 4 / (ms * 1e-3) / HBM_COPY, 3) if ms > 0 else None
        print(json.dumps(row), flush=True)
        steps.append(row)
    out = {"steps": steps}
    if args.fit:
        out["fit"] = run_child(args, ["--child", "fit"])
        if out["fit"] is None:
            return 1
        for r in out["fit"]:
            print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
