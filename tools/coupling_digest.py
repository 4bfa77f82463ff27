"""SHA-256 digests of what the conditioner-network (coupling) kernels write (nf_pack.h, nf_coupling.hip, nf_deep.hip, nf_wide.hip,
nf_rqs.hip), for a bit-for-bit comparison of two builds of libnfhip.so (run once per library, each run its own process, then
compare the two files with --compare).  Cases: the `netgeo`, `deep` and `wide` shapes of tests/affine_cases.py and the RQS_FUSED
shapes of tests/spline_cases.py, each with the case table's own layer count and theta (gain = 1), at N = 33 (two tiles, the second
ragged) and N = 6 753 (212 tiles with a ragged last one: 53 reverse-pass workgroups, the smallest slab count at which the 8 W
arm, the 4 W arm and the remainder of the slab sum all run).  Per case and N:
  fwd / inv     -- nf_flow_fwd and nf_flow_inv: outputs and ladj,
  vg_diag, vg_banana
                -- nf_elbo_value_and_grad with in-library draws on the diagonal-Gaussian target and on Banana: gradient, loss and
                   the whole caller arena the call worked in (zeroed beforehand),
  fkl           -- nf_loglikelihood_value_and_grad: the same three,
  elbo_step, fkl_step
                -- two nf_elbo_step / nf_loglikelihood_step calls: theta, m, v and the arena.
A call the library refuses is recorded by its message.  The retained A/B kernel forms run only under an environment switch, read
once per process: set the switch in the environment of the run (--switch-sets prints the sets the regime tests exercise, one per
line, with the cases each concerns as a --only argument).
The arena digests of the LDS-resident shapes are NOT a function of the library: the reverse kernels write a workgroup's slab as whole
padded images, 16 bytes at a time, and the NF_IMG_PAD columns behind each weight row carry whatever the LDS region held before the
fold (no kernel reads them back: they have no theta index).  --arena-dir DIR keeps every arena of a run (compressed), --shapes
restricts the run, and --compare-arenas A1 A2 B, for two runs of one library and one of the other, lists per entry and call where
A1 differs from A2 and from B, in 16-byte cells, and fails if B leaves the regions in which the library differs from itself (with
many slabs it does: which slabs come out different varies from run to run; DESIGN.md, "The conditioner-network kernels' shared stages").
--lib PATH digests another build (tools/simple_step_digest.py's convention: loaded instead of the in-tree one, never copied over it).
usage: python tools/coupling_digest.py [--lib PATH] [--only affine|spline] out.json
       python tools/coupling_digest.py --compare a.json b.json
       python tools/coupling_digest.py --switch-sets
       python tools/coupling_digest.py --compare-arenas DIR_A1 DIR_A2 DIR_B"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

NS = (33, 6753)
SEED = 77
FAMILY_SWITCH = ("NF_AFFINE_", "NF_BWD_", "NF_FWD_", "NF_STASH_", "NF_WIDE_", "NF_DEEP_", "NF_RQS_")  # switches that reach this family


def switch_sets():
    """[(switches, 'affine' | 'spline')] of the rows of the two regime tests that select kernels of this family"""
    import test_gpu_affine_regimes as ta
    import test_gpu_spline_regimes as ts

    out = []
    for only, rows in (("affine", ta.ROWS), ("spline", ts.ROWS)):
        for sw, _ in rows.values():
            if all(s.startswith(FAMILY_SWITCH) for s in sw) and (only == "affine") != any(s.startswith("NF_RQS_") for s in sw) \
                    and (tuple(sw), only) not in out:
                out.append((tuple(sw), only))
    return out


def compare(a, b):
    with open(a) as f:
        ja = json.load(f)
    with open(b) as f:
        jb = json.load(f)
    ja.pop("lib"), jb.pop("lib")
    keys = sorted(set(ja) | set(jb))
    differ = [k for k in keys if ja.get(k) != jb.get(k)]

    def fields(k, call):
        x, y = (ja.get(k) or {}).get(call) or {}, (jb.get(k) or {}).get(call) or {}
        return [f for f in sorted(set(x) | set(y)) if x.get(f) != y.get(f)]

    outputs = [k for k in differ if any(f != "arena" for call in set(ja.get(k) or {}) | set(jb.get(k) or {}) for f in fields(k, call))]
    refused = sum(1 for k in keys for call in (ja.get(k) or {}).values() if "refused" in call)
    digests = sum(len(call) for k in keys for call in (ja.get(k) or {}).values())
    print(f"{os.path.basename(a)} vs {os.path.basename(b)}: {len(keys)} entries, {digests} digests, {refused} refused calls, {len(differ)} entries differ"
          f" ({len(outputs)} in an output, {len(differ) - len(outputs)} in the arena only)")
    for k in differ:
        calls = sorted(set(ja.get(k) or {}) | set(jb.get(k) or {}))
        print(f"  differs: {k}: " + ", ".join(f"{c} [{' '.join(fields(k, c))}]" for c in calls if fields(k, c)))
    return 1 if differ else 0


def compare_arenas(a1, a2, b):
    """per arena kept by three runs: the 16-byte cells in which A1 differs from A2 (one library against itself) and from B (the other
    library), and the regions they lie in (cells less than 64 KiB apart are one region)"""
    import numpy as np

    def cells(x, y):
        n = min(len(x), len(y)) // 16 * 16
        return np.nonzero((x[:n].reshape(-1, 16) != y[:n].reshape(-1, 16)).any(axis=1))[0]

    def regions(c):
        if not len(c):
            return []
        cut = np.nonzero(np.diff(c) > 4096)[0]
        return [(int(lo) * 16, int(hi) * 16 + 16) for lo, hi in zip(np.r_[c[0], c[cut + 1]], np.r_[c[cut], c[-1]])]

    bad = 0
    for name in sorted(os.listdir(a1)):
        x, y, z = (np.load(os.path.join(d, name))["a"] for d in (a1, a2, b))
        same_size = len(x) == len(y) == len(z)
        self_c, other_c = cells(x, y), cells(x, z)
        rs = regions(self_c)
        outside = [int(c) * 16 for c in other_c if not any(lo - 4096 * 16 <= c * 16 < hi + 4096 * 16 for lo, hi in rs)]
        bad += bool(outside) or not same_size
        print(f"{name[:-4]}: {len(x)} bytes; A1 vs A2 {len(self_c)} cells in {rs if len(rs) <= 4 else str(rs[:4]) + ' ...'}; A1 vs B {len(other_c)} cells, "
              f"{len(np.setdiff1d(other_c, self_c))} of them equal in A1 and A2, {len(outside)} outside A's own regions"
              + ("" if same_size else "; SIZES DIFFER") + (f": first at byte {outside[0]}" if outside else ""))
    print(f"arenas whose differences from B leave the regions in which A differs from itself: {bad}")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default="")
    ap.add_argument("--only", choices=("affine", "spline"), default="")
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--switch-sets", action="store_true")
    ap.add_argument("--compare-arenas", action="store_true")
    ap.add_argument("--arena-dir", default="")
    ap.add_argument("--shapes", default="", help="comma-separated shape names: only these cases")
    ap.add_argument("files", nargs="*")
    args = ap.parse_args()
    if args.switch_sets:
        for sw, only in switch_sets():
            print(" ".join(f"{s}=1" for s in sw) + f" --only {only}")
        return 0
    if args.compare:
        return compare(*args.files)
    if args.compare_arenas:
        return compare_arenas(*args.files)
    (out_path,) = args.files

    import torch

    import affine_cases as A
    import spline_cases as S
    from __graft_entry__ import load_package
    from simple_step_digest import sha, vp

    nf = load_package()
    if args.lib:
        nf._lib.LIB_PATH = os.path.abspath(args.lib)
    lib = nf.load_library()
    check = nf._lib.check
    dt = torch.float32

    def flows():
        """(name, flow, diagonal-Gaussian target) of every case"""
        if args.only != "spline":
            for shape, fam in A.FAMILY.items():
                if fam in ("netgeo", "deep", "wide") and (not args.shapes or shape in args.shapes.split(",")):
                    flow, tgt, _ = A.make_flow(nf, A.case(shape, 1), torch)
                    yield shape, flow, tgt
        if args.only != "affine":
            for shape in (s for s in S.RQS_FUSED if not args.shapes or s in args.shapes.split(",")):
                c = S.case(shape, 1)
                b = S.build(c)
                flow = nf.Flow("nsf", nf.MvNormal(c.d), 1, c.hdims, c.K, c.B, dtype=dt, device="cuda", theta=torch.tensor(b.th, dtype=dt, device="cuda"))
                yield shape, flow, nf.DiagGaussTarget(torch.tensor(b.mu, dtype=dt, device="cuda"), torch.tensor(b.var, dtype=dt, device="cuda"))

    def with_arena(flow, n, fn):
        """fn(ctx) on a fresh context that works in a zeroed caller arena; returns the arena's digest"""
        ctx = nf.Context(0, torch.cuda.current_stream().cuda_stream)
        need = int(lib.nf_workspace_bytes(ctx.ptr, C.byref(flow.desc), n))
        arena = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
        check(lib.nf_ctx_set_arena(ctx.ptr, C.c_void_p((arena.data_ptr() + 255) // 256 * 256), need))
        try:
            fn(ctx)
            torch.cuda.synchronize()
        finally:
            check(lib.nf_ctx_set_arena(ctx.ptr, None, 0))
            ctx.close()
        if args.arena_dir:
            import numpy as np

            os.makedirs(args.arena_dir, exist_ok=True)
            np.savez_compressed(os.path.join(args.arena_dir, "__".join(current) + ".npz"), a=arena.cpu().numpy())
        return sha(arena)

    current = ["", ""]  # entry and call that is running, for --arena-dir

    def call(row, name, fn):
        current[1] = name
        try:
            row[name] = fn()
        except nf.NFHipError as e:
            row[name] = {"refused": str(e)}

    res = {"lib": "--lib" if args.lib else "in-tree"}  # which build, not where it lay
    for shape, flow, tgt in flows():
        d, P, desc, th = flow.desc.d, flow.P, C.byref(flow.desc), flow.theta
        banana = nf.BananaTarget(d, 0.1, 4.0)
        for n in NS:
            row = {}
            current[0] = f"{shape}_N{n}"
            xs = nf.device_specific_rand(nf.PhiloxRNG(17), nf.MvNormal(d), n, dtype=dt)
            ys = nf.device_specific_rand(nf.PhiloxRNG(5), nf.MvNormal(d), n, dtype=dt).mul_(0.7)

            def apply(fn, x):
                y, ladj = torch.zeros_like(x), torch.zeros(n, dtype=dt, device="cuda")
                ws = with_arena(flow, n, lambda ctx: check(fn(ctx.ptr, desc, vp(th), vp(x), n, vp(y), vp(ladj))))
                return {"y": sha(y), "ladj": sha(ladj), "arena": ws}

            def vg(target):
                out = torch.zeros(P + 1, dtype=dt, device="cuda")
                ws = with_arena(flow, n, lambda ctx: check(lib.nf_elbo_value_and_grad(ctx.ptr, desc, C.byref(target.c), vp(th), None, n, n, SEED, 0, 0, vp(out))))
                return {"grad": sha(out[:P]), "loss": sha(out[P:]), "arena": ws}

            def fkl():
                out = torch.zeros(P + 1, dtype=dt, device="cuda")
                ws = with_arena(flow, n, lambda ctx: check(lib.nf_loglikelihood_value_and_grad(ctx.ptr, desc, vp(th), vp(ys), n, n, vp(out))))
                return {"grad": sha(out[:P]), "loss": sha(out[P:]), "arena": ws}

            def steps(one):
                t, m, v = th.clone(), torch.zeros_like(th), torch.zeros_like(th)
                loss, gnorm = C.c_double(0), C.c_double(0)

                def two(ctx):
                    for step in (0, 1):
                        check(one(ctx, t, m, v, step, loss, gnorm))

                ws = with_arena(flow, n, two)
                return {"theta": sha(t), "m": sha(m), "v": sha(v), "loss": loss.value.hex(), "gnorm": gnorm.value.hex(), "arena": ws}

            call(row, "fwd", lambda: apply(lib.nf_flow_fwd, xs))
            call(row, "inv", lambda: apply(lib.nf_flow_inv, ys))
            call(row, "vg_diag", lambda: vg(tgt))
            call(row, "vg_banana", lambda: vg(banana))
            call(row, "fkl", fkl)
            call(row, "elbo_step", lambda: steps(lambda ctx, t, m, v, step, loss, gnorm: lib.nf_elbo_step(
                ctx.ptr, desc, C.byref(tgt.c), vp(t), vp(m), vp(v), n, SEED, step, 1e-3, 0.9, 0.999, 1e-8, C.byref(loss), C.byref(gnorm))))
            call(row, "fkl_step", lambda: steps(lambda ctx, t, m, v, step, loss, gnorm: lib.nf_loglikelihood_step(
                ctx.ptr, desc, vp(t), vp(m), vp(v), vp(ys), n, n, step, 1e-3, 0.9, 0.999, 1e-8, C.byref(loss), C.byref(gnorm))))
            res[f"{shape}_N{n}"] = row
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    refused = sum(1 for row in res.values() if isinstance(row, dict) for c in row.values() if "refused" in c)
    print(f"{len(res) - 1} entries ({refused} refused calls) -> {out_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
