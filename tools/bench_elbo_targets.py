"""ms per reverse-KL training iteration (train_flow(elbo_batch, flow, target, n) with Adam) on the built-in targets other than
the diagonal Gaussian, three ways:
  split  -- `optimize` over value_and_gradient + update (two host reads per iteration),
  step   -- one nf_elbo_step per iteration (asynchronous: no host read),
  graph  -- replay of a captured nf_elbo_step_enqueue (None where the library answers NF_ERR_UNSUPPORTED).
Cases: (a) realnvp(q0, [16, 16], 3) on Banana(2, 1, 100) with 16 samples (example/demo_RealNVP.jl as written), (b) the cfg-2 flow
(d = 64, hidden [64, 64], 8 couplings, 65 536 samples) on Banana(64) and Funnel(64), (c) the cfg-3 flow (NSF d = 32, K = 8,
131 072 samples) on Funnel(32), (d) nsf d = 2 on Cross.
Every figure is the median of --runs timed loops after a clock ramp of --ramp seconds of steps (bench.py's pre-warm convention);
the spread (max - min) is printed next to it.  --lib PATH times another build of libnfhip.so (an A/B against an older commit:
build it in a separate checkout and pass its library here; it is loaded instead of the in-tree one, never copied over it).
usage: python tools/bench_elbo_targets.py [--runs 3] [--case a,b,...] [--lib PATH]"""
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
    iters = max(min_iters, min(2000, int(seconds / max(time.perf_counter() - t0, 1e-6))))
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
    f32 = torch.float32
    cases = [
        ("a_demo_realnvp_d2_h16x6", "banana", lambda: nf.realnvp(q(2), (16, 16), 3, paramtype=f32, seed=1), lambda: nf.BananaTarget(2, 1.0, 100.0), 16),
        ("b_cfg2_realnvp_d64_h64x8", "banana", lambda: nf.realnvp(q(64), (64, 64), 4, paramtype=f32, seed=1), lambda: nf.BananaTarget(64, 1.0, 100.0), 65536),
        ("b_cfg2_realnvp_d64_h64x8", "funnel", lambda: nf.realnvp(q(64), (64, 64), 4, paramtype=f32, seed=1), lambda: nf.FunnelTarget(64, 0.0, 9.0), 65536),
        ("c_cfg3_nsf_d32_k8x8", "funnel", lambda: nf.nsf(q(32), (32, 32), 8, 5.0, 4, paramtype=f32, seed=1), lambda: nf.FunnelTarget(32, 0.0, 9.0), 131072),
        ("d_nsf_d2_k8x4", "cross", lambda: nf.nsf(q(2), (32, 32), 8, 5.0, 2, paramtype=f32, seed=1), lambda: nf.CrossTarget(2.0, 0.15), 4096),
    ]
    want = [c for c in args.case.split(",") if c]
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for name, tname, make, make_tgt, n in cases:
        if want and name[0] not in want:
            continue
        flow, tgt = make(), make_tgt()
        theta0, re = flow.destructure()
        row = {"flow": name, "target": tname, "N": n, "lib": args.lib or "in-tree"}
        ctx = flow.ctx
        nf._lib.check(lib.nf_ctx_set_weight_cache(ctx.ptr, 1))
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
        nf._lib.check(lib.nf_ctx_set_weight_cache(ctx.ptr, 0))
        th2 = theta0.clone()
        st = nf.setup(nf.Adam(LR), th2)
        rng = nf.PhiloxRNG(7)

        def split():
            ls, g = nf.value_and_gradient(nf.elbo_batch, re(th2), tgt, n, rng)
            float(nf.update(nf.Adam(LR), st, th2, g))

        split()
        row["split_ms"], row["split_spread"] = stats(split, args.runs)
        counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        gctx = nf.Context(0, side.cuda_stream)
        nf._lib.check(lib.nf_ctx_set_weight_cache(gctx.ptr, 1))
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
        del flow, th, m, v, th2, th3, m3, v3
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
