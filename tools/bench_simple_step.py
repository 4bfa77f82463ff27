"""ms per reverse-KL training iteration of planar and radial flows (train_flow(elbo_batch, flow, target, n) with Adam), three ways:
  split  -- nf_elbo_value_and_grad + nf_adam_update per iteration (asynchronous: no host read),
  step   -- one nf_elbo_step per iteration (asynchronous: no host read),
  graph  -- replay of a captured nf_elbo_step_enqueue (None where the library answers NF_ERR_UNSUPPORTED).
Shapes: (a) BASELINE cfg 1 -- planarflow d = 2, 10 layers, Float64, 1024 samples, Banana(2, 1, 10); (b) the same flow at the 32
samples of example/demo_planar_flow.jl; (c) radialflow d = 2, 10 layers, Float64, 32 samples (example/demo_radial_flow.jl);
(d) planarflow d = 64, 10 layers, Float32, 65 536 samples, Banana(64, 1, 10); (e) radialflow d = 64, 10 layers, Float32, 65 536 samples,
Banana(64, 1, 10): a two-block k_radial_step outside the diagonal-Gaussian instantiation; (f) the planar flow of (d) with the
Banana target named in the case (the shape of (d), whose target is Banana already: a second reading of that shape).
Every figure is the median of --runs timed loops after a clock ramp of --ramp seconds of steps (bench.py's pre-warm convention);
the spread (max - min) is printed next to it.  --lib PATH times another build of libnfhip.so (an A/B against an older commit:
build it in a separate checkout and pass its library here; it is loaded instead of the in-tree one, never copied over it).
usage: python tools/bench_simple_step.py [--runs 3] [--case a,b,...] [--lib PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def timed(fn, seconds=0.25, min_iters=5):
    """ms per call over a loop sized to last about `seconds`"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    iters = max(min_iters, min(5000, int(seconds / max(time.perf_counter() - t0, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def stats(fn, runs):
    v = [timed(fn) for _ in range(runs)]
    return round(statistics.median(v), 4), round(max(v) - min(v), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ramp", type=float, default=1.0)
    ap.add_argument("--case", default="")
    ap.add_argument("--lib", default="")
    args = ap.parse_args()
    nf = load_package()
    if args.lib:
        nf._lib.LIB_PATH = os.path.abspath(args.lib)
    lib = nf.load_library()
    q = lambda d: nf.MvNormal(d)  # noqa: E731
    f32, f64 = torch.float32, torch.float64
    scaled = lambda f: f.with_theta(f.theta * 0.3)  # noqa: E731
    cases = [
        ("a_cfg1_planar_d2x10_f64", lambda: scaled(nf.planarflow(q(2), 10, paramtype=f64, seed=1)), lambda: nf.BananaTarget(2, 1.0, 10.0), 1024),
        ("b_demo_planar_d2x10_f64", lambda: scaled(nf.planarflow(q(2), 10, paramtype=f64, seed=1)), lambda: nf.BananaTarget(2, 1.0, 10.0), 32),
        ("c_demo_radial_d2x10_f64", lambda: scaled(nf.radialflow(q(2), 10, paramtype=f64, seed=1)), lambda: nf.BananaTarget(2, 1.0, 10.0), 32),
        ("d_planar_d64x10_f32", lambda: scaled(nf.planarflow(q(64), 10, paramtype=f32, seed=1)), lambda: nf.BananaTarget(64, 1.0, 10.0), 65536),
        ("e_radial_d64x10_f32_banana", lambda: scaled(nf.radialflow(q(64), 10, paramtype=f32, seed=1)), lambda: nf.BananaTarget(64, 1.0, 10.0), 65536),
        ("f_planar_d64x10_f32_banana", lambda: scaled(nf.planarflow(q(64), 10, paramtype=f32, seed=1)), lambda: nf.BananaTarget(64, 1.0, 10.0), 65536),
    ]
    want = [c for c in args.case.split(",") if c]
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for name, make, make_tgt, n in cases:
        if want and name[0] not in want:
            continue
        flow, tgt = make(), make_tgt()
        theta0 = flow.theta.clone()
        dcode = 0 if theta0.dtype == f32 else 1
        row = {"flow": name, "N": n, "lib": args.lib or "in-tree"}
        ctx = flow.ctx
        th = theta0.clone()
        m, v = torch.zeros_like(th), torch.zeros_like(th)
        k = [0]

        def step():
            nf._lib.check(lib.nf_elbo_step(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, 7, k[0], LR, B1, B2, EPS, None, None))
            k[0] += 1

        step()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.ramp:  # clock ramp
            step()
        torch.cuda.synchronize()
        row["step_ms"], row["step_spread"] = stats(step, args.runs)
        th2 = theta0.clone()
        m2, v2 = torch.zeros_like(th2), torch.zeros_like(th2)
        out = torch.empty(flow.P + 1, dtype=theta0.dtype, device="cuda")
        gn = torch.empty(1, dtype=theta0.dtype, device="cuda")
        k2 = [0]

        def split():
            nf._lib.check(lib.nf_elbo_value_and_grad(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th2), None, n, n, 7, 0, k2[0], vp(out)))
            nf._lib.check(lib.nf_adam_update(ctx.ptr, dcode, vp(th2), vp(out), vp(m2), vp(v2), flow.P, LR, B1, B2, EPS, k2[0] + 1, vp(gn)))
            k2[0] += 1

        split()
        row["split_ms"], row["split_spread"] = stats(split, args.runs)
        counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        gctx = nf.Context(0, side.cuda_stream)
        th3 = theta0.clone()
        m3, v3 = torch.zeros_like(th3), torch.zeros_like(th3)

        def enqueue():
            return lib.nf_elbo_step_enqueue(gctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th3), vp(m3), vp(v3), n, 7, vp(counter), LR, B1, B2,
                                            EPS, None)

        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            code = enqueue()
        side.synchronize()
        if code == 0:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                nf._lib.check(enqueue())
            row["graph_ms"], row["graph_spread"] = stats(graph.replay, args.runs)
            del graph
        else:
            row["graph_ms"] = None  # this library has no graph form for the case
        gctx.close()
        print(json.dumps(row), flush=True)
        del flow, th, m, v, th2, m2, v2, th3, m3, v3
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
