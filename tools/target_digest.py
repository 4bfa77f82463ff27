"""SHA-256 digests of what the matrix-pipe target kernels write (nf_linpred.hip, nf_mixture.hip, nf_softmax.hip, nf_bnn.hip,
nf_ordinal.hip, nf_riskset.hip), for a bit-for-bit comparison of two builds of libnfhip.so (run once per library, each run its own
process, then compare the two files).  Every kind of the six families, at the shapes of the GPU tests' own tables plus, where the
tables stop short, one d in each of <= 32, 33..64, 65..128 and > 128; N = 33 samples (two tiles with a ragged second, three flat
blocks with a ragged third); 33 data rows where the target takes any row count.  Per case and element type:
  logp          -- nf_target_logp with its gradient (the flat kernel: logp_out, grad_out),
  elbo_batch    -- nf_elbo_batch through a full-rank flow: the per-sample terms and the mean (elbos_out and the partials),
  vg            -- nf_elbo_value_and_grad through the same flow: gradient, loss, and the whole caller arena the call worked in
                   (zeroed beforehand: the target's gradient tile and the partials of every block).
The Float32 flow reaches the tiled kernel, the Float64 flow the flat one.  A call the library refuses is recorded by its message.
--lib PATH digests another build (tools/simple_step_digest.py's convention: loaded instead of the in-tree one, never copied over it).
usage: python tools/target_digest.py [--lib PATH] out.json"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
from __graft_entry__ import load_package  # noqa: E402
from simple_step_digest import sha, vp  # noqa: E402

N, ROWS, SEED = 33, 33, 77
WIDE = (100, 200)  # a d in 65..128 and one beyond 128, for the families whose tables stop at 64


def cases(nf, f64):
    """(name, d, function that builds the target in the element type) of every case"""
    import bnn_forms as bf
    import disp_forms as df
    import glm_forms as gf
    import hier_forms as hf
    import ordinal_forms as of
    import riskset_forms as rf
    import softmax_forms as sf
    import test_gpu_bnn as tb
    import test_gpu_glm as tg
    import test_gpu_linpred as tl
    import test_gpu_mixture as tm
    import test_gpu_ordinal as to
    import test_gpu_riskset as tr
    import test_gpu_softmax as ts

    dt = tl.tdt(f64)
    out = []
    for d in (5, 64) + WIDE:
        out.append((f"gauss_d{d}", d, lambda d=d: tl.make_gauss(nf, d, f64)[0]))
        out.append((f"logreg_d{d}", d, lambda d=d: tl.make_logreg(nf, d, ROWS, f64)[0]))
        out.append((f"logreg_shift_d{d}", d, lambda d=d: tl.make_logreg(nf, d, ROWS, f64, shift=True)[0]))
        for fam in gf.FAMILIES:
            out.append((f"glm_{fam}_d{d}", d, lambda d=d, fam=fam: tg.make_glm(nf, fam, d, ROWS, f64)[0]))
    for d, G in hf.SHAPES[1:] + [(w, 8) for w in WIDE]:
        for fam in hf.FAMILIES:
            out.append((f"hglm_{fam}_d{d}_G{G}", d, lambda d=d, G=G, fam=fam: hf.build(nf, fam, d, G, ROWS, dt, "cuda", 5)))
    for d, G in df.SHAPES[1:] + [(w, 8) for w in WIDE]:
        for fam in df.FAMILIES:
            out.append((f"dglm_{fam}_d{d}_G{G}", d, lambda d=d, G=G, fam=fam: df.build(nf, fam, d, G, ROWS, dt, "cuda", 5, 18, None)))
    for d, K in ((5, 3), (33, 5), (64, 9)):
        out.append((f"mixture_d{d}_K{K}", d, lambda d=d, K=K: tm.make_mixture(nf, d, K, f64)[0]))
    for shape in sf.SHAPES:
        out.append(("softmax_C%d_p%d_r%d" % shape, shape[0] * shape[1], lambda shape=shape: ts.make_softmax(nf, shape, f64)[0]))
    for fam in bf.FAMILIES:
        for shape in bf.SHAPES:
            out.append((f"bnn_{fam}_H%d_p%d_r%d" % shape, bf.dim(shape[0], shape[1]), lambda fam=fam, shape=shape: tb.make_bnn(nf, fam, shape, f64)[0]))
    for shape in of.SHAPES:
        out.append(("ordinal_C%d_p%d_r%d" % shape, of.dim(shape[0], shape[1]), lambda shape=shape: to.make_ordinal(nf, shape, f64)[0]))
    for case in rf.CASES:
        out.append(("riskset_%s_d%d" % case, case[1], lambda case=case: tr.make_riskset(nf, case, f64)[0]))
    return out


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
    import test_gpu_ordinal as to

    def with_arena(flow, fn):
        """fn(ctx) on a fresh context that works in a zeroed caller arena; returns the arena's digest"""
        ctx = nf.Context(0, torch.cuda.current_stream().cuda_stream)
        need = int(lib.nf_workspace_bytes(ctx.ptr, C.byref(flow.desc), N))
        arena = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
        check(lib.nf_ctx_set_arena(ctx.ptr, C.c_void_p((arena.data_ptr() + 255) // 256 * 256), need))
        try:
            fn(ctx)
            torch.cuda.synchronize()
        finally:
            check(lib.nf_ctx_set_arena(ctx.ptr, None, 0))
            ctx.close()
        return sha(arena)

    res, refused = {"lib": "--lib" if args.lib else "in-tree"}, 0  # which build, not where it lay
    for f64 in (False, True):
        dt, tag = (torch.float64, "f64") if f64 else (torch.float32, "f32")
        for name, d, build in cases(nf, f64):
            row = {}
            y = nf.device_specific_rand(nf.PhiloxRNG(5), nf.MvNormal(d), N, dtype=dt)
            y.mul_(0.3)
            xs = nf.device_specific_rand(nf.PhiloxRNG(17), nf.MvNormal(d), N, dtype=dt)
            flow = to.fullrank_flow(nf, d, f64, to.fullrank_theta(d))
            try:
                tgt = build()
                lp, g = nf.target_logp(tgt, y, with_grad=True)
                torch.cuda.synchronize()
                row["logp"] = {"logp": sha(lp), "grad": sha(g)}
                elbos, mean = torch.zeros(N, dtype=dt, device="cuda"), C.c_double(0)
                ws = with_arena(flow, lambda ctx: check(lib.nf_elbo_batch(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(flow.theta), vp(xs), N,
                                                                          vp(elbos), C.byref(mean))))
                row["elbo_batch"] = {"elbos": sha(elbos), "mean": mean.value.hex(), "arena": ws}
                out = torch.zeros(flow.P + 1, dtype=dt, device="cuda")
                ws = with_arena(flow, lambda ctx: check(lib.nf_elbo_value_and_grad(ctx.ptr, C.byref(flow.desc), C.byref(tgt.c), vp(flow.theta),
                                                                                   vp(xs), N, N, SEED, 0, 0, vp(out))))
                row["vg"] = {"grad": sha(out[:flow.P]), "loss": sha(out[flow.P:]), "arena": ws}
            except nf.NFHipError as e:
                row["refused"] = str(e)
                refused += 1
            res[f"{name}_{tag}"] = row
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(res) - 1} entries ({refused} with a refused call) -> {args.out}")


if __name__ == "__main__":
    main()
