"""ms per forward-KL training iteration (train_flow(loglikelihood, flow, xs) with Adam), three ways:
  split  -- `optimize` over loglikelihood_value_and_gradient + update (two host reads per iteration),
  step   -- one nf_loglikelihood_step per iteration (asynchronous: no host read),
  graph  -- replay of a captured nf_loglikelihood_step_enqueue (flows with the fused form only).
Flows: BASELINE cfg 5's (d = 64, 8 couplings, hidden [64, 64]) at N = 65 536 and 1 048 576, cfg 3's NSF at 131 072.
usage: python tools/bench_fkl_step.py [--iters K]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def timed(fn, iters):
    fn()  # warm-up (workspace, kernel attributes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    nf = load_package()
    lib = nf.load_library()
    cases = [("cfg5_realnvp_d64_h64x8", lambda: nf.realnvp(nf.MvNormal(64), (64, 64), 4, paramtype=torch.float32, seed=1), 65536),
             ("cfg5_realnvp_d64_h64x8", lambda: nf.realnvp(nf.MvNormal(64), (64, 64), 4, paramtype=torch.float32, seed=1), 1048576),
             ("cfg3_nsf_d32_k8", lambda: nf.nsf(nf.MvNormal(32), (32, 32), 8, 5.0, 4, paramtype=torch.float32, seed=1), 131072)]
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for name, make, n in cases:
        flow = make()
        d = flow.dist.d
        xs = torch.randn(n, d, device="cuda").t()  # d x N column-major
        theta0, re = flow.destructure()
        row = {"flow": name, "N": n}
        th = theta0.clone()
        st = nf.setup(nf.Adam(LR), th)

        def split():
            ls, g = nf.loglikelihood_value_and_gradient(re(th), xs)
            float(nf.update(nf.Adam(LR), st, th, g))

        row["split_ms"] = round(timed(split, args.iters), 4)
        ctx = flow.ctx
        th = theta0.clone()
        m, v = torch.zeros_like(th), torch.zeros_like(th)
        k = [0]
        nf._lib.check(lib.nf_ctx_set_weight_cache(ctx.ptr, 1))

        def step():
            nf._lib.check(lib.nf_loglikelihood_step(ctx.ptr, C.byref(flow.desc), vp(th), vp(m), vp(v), vp(xs), n, n, k[0], LR, B1, B2, EPS,
                                                    None, None))
            k[0] += 1

        row["step_ms"] = round(timed(step, args.iters), 4)
        counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        gctx = nf.Context(0, side.cuda_stream)
        nf._lib.check(lib.nf_ctx_set_weight_cache(gctx.ptr, 1))

        def enqueue():
            return lib.nf_loglikelihood_step_enqueue(gctx.ptr, C.byref(flow.desc), vp(th), vp(m), vp(v), vp(xs), n, n, vp(counter), LR, B1,
                                                     B2, EPS, None)

        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            code = enqueue()
        side.synchronize()
        if code == 0:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                nf._lib.check(enqueue())
            row["graph_ms"] = round(timed(graph.replay, args.iters), 4)
        else:
            row["graph_ms"] = None  # no fused form for this flow
        nf._lib.check(lib.nf_ctx_set_weight_cache(ctx.ptr, 0))
        gctx.close()
        print(json.dumps(row), flush=True)
        del flow, xs, th, m, v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
