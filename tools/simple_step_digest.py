"""SHA-256 digests of what the planar / radial / mean-field step kernels and the element-wise target kernels write, for a
bit-for-bit comparison of two builds of libnfhip.so (run once per library, then compare the two files).
For the nine CASES of tests/test_gpu_simple_step.py and the TILE_CASES of tests/test_gpu_parity.py, each call on a fresh context:
  vg_rng / vg_xs -- nf_elbo_value_and_grad with in-library draws and with supplied draws: gradient, loss, and the whole
                    caller arena the call worked in (zeroed beforehand: the loss partials of every block and the gradient slabs),
  elbo_batch     -- nf_elbo_batch: the per-sample terms and the mean,
  step2          -- theta, m and v after two nf_elbo_step calls;
and nf_target_logp with its gradient for the five element-wise kinds in both element types.
--lib PATH digests another build (tools/bench_simple_step.py's convention: loaded instead of the in-tree one, never copied
over it).
usage: python tools/simple_step_digest.py [--lib PATH] out.json"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
from __graft_entry__ import load_package  # noqa: E402

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
SEED = 77


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="")
    ap.add_argument("out")
    args = ap.parse_args()
    nf = load_package()
    if args.lib:
        nf._lib.LIB_PATH = os.path.abspath(args.lib)
    lib = nf.load_library()
    check = nf._lib.check
    import test_gpu_parity as tp
    import test_gpu_simple_step as ts

    cases = {name: ts.make_case(nf, name) for name in ts.CASES}
    for kind, d, nl, tname in tp.TILE_CASES:
        flow, tgt = tp.tile_case(nf, kind, d, nl, tname)[:2]
        cases[f"tile_{kind}_d{d}x{nl}_{tname}"] = (flow, tgt, tp.TILE_N)
    res = {"lib": "--lib" if args.lib else "in-tree"}  # which build, not where it lay

    def with_arena(flow, n, fn):
        """fn(ctx) on a fresh context that works in a zeroed caller arena; returns (fn's result, the arena's digest)"""
        ctx = nf.Context(0, torch.cuda.current_stream().cuda_stream)
        need = int(lib.nf_workspace_bytes(ctx.ptr, C.byref(flow.desc), n))
        arena = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
        check(lib.nf_ctx_set_arena(ctx.ptr, C.c_void_p((arena.data_ptr() + 255) // 256 * 256), need))
        try:
            out = fn(ctx)
            torch.cuda.synchronize()
        finally:
            check(lib.nf_ctx_set_arena(ctx.ptr, None, 0))
            ctx.close()
        return out, sha(arena)

    for name, (flow, tgt, n) in cases.items():
        dt, P = flow.theta.dtype, flow.P
        xs = nf.device_specific_rand(nf.PhiloxRNG(17), flow.dist, n, dtype=dt)
        row = {}
        for form, x in (("vg_rng", None), ("vg_xs", xs)):
            out = torch.zeros(P + 1, dtype=dt, device="cuda")
            _, ws = with_arena(flow, n, lambda ctx: check(lib.nf_elbo_value_and_grad(
                ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(flow.theta), vp(x), n, n, SEED, 0, 0, vp(out))))
            row[form] = {"grad": sha(out[:P]), "loss": sha(out[P:]), "arena": ws}
        elbos, mean = torch.zeros(n, dtype=dt, device="cuda"), C.c_double(0)
        with_arena(flow, n, lambda ctx: check(lib.nf_elbo_batch(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(flow.theta), vp(xs), n,
                                                                vp(elbos), C.byref(mean))))
        row["elbo_batch"] = {"elbos": sha(elbos), "mean": mean.value.hex()}
        th, m, v = flow.theta.clone(), torch.zeros_like(flow.theta), torch.zeros_like(flow.theta)

        def two_steps(ctx):
            for step in range(2):
                check(lib.nf_elbo_step(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(th), vp(m), vp(v), n, SEED, step, LR, B1, B2, EPS,
                                       None, None))

        with_arena(flow, n, two_steps)
        row["step2"] = {"theta": sha(th), "m": sha(m), "v": sha(v)}
        res[name] = row
    for dt in (torch.float32, torch.float64):
        gen = torch.Generator().manual_seed(6)
        mu, var = torch.randn(6, generator=gen, dtype=torch.float64), torch.rand(6, generator=gen, dtype=torch.float64) + 0.5
        targets = {"diaggauss": (6, nf.DiagGaussTarget(mu.to(dt).cuda(), var.to(dt).cuda())), "banana": (6, nf.BananaTarget(6, 0.3, 4.0)),
                   "funnel": (6, nf.FunnelTarget(6, 0.3, 2.0)), "warped": (2, nf.WarpedGaussTarget(1.0, 0.12)),
                   "cross": (2, nf.CrossTarget(2.0, 0.15))}
        for tname, (d, tgt) in targets.items():
            y = nf.device_specific_rand(nf.PhiloxRNG(5), nf.MvNormal(d), 333, dtype=dt)
            y.mul_(1.2)
            lp, g = nf.target_logp(tgt, y, with_grad=True)
            torch.cuda.synchronize()
            res[f"target_logp_{tname}_{str(dt).split('.')[-1]}"] = {"logp": sha(lp), "grad": sha(g)}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(res) - 1} entries -> {args.out}")


if __name__ == "__main__":
    main()
