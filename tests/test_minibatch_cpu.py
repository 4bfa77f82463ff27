"""CPU checks of the row-minibatch target (nf_target_minibatch, MinibatchTarget): the sampling rule in numpy over the oracle's Philox
(strata, ranges, the identity at m = R, row frequencies), each kind's segment table against the packed buffer, the constructor's
refusals, the new symbol with the ABI, the symbol list and the descriptor unchanged, the entry point's argument errors BEFORE any
device work (a stand-in context and host buffers that must stay untouched), and the new kernels' resources."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import minibatch_ref as mr
from __graft_entry__ import ROOT, SOURCES, build, load_package


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


# ---- the sampling rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,m", [(77, 1), (77, 7), (77, 33), (77, 77), (8, 2), (40, 9), (5, 2), (6, 3), (2**31 - 1, 3), (131072, 1024)])
def test_strata_partition_the_rows(R, m):
    lo, n = mr.strata(R, m)
    assert lo[0] == 0 and lo[-1] == R and (n >= 1).all() and n.sum() == R
    assert n.max() - n.min() <= 1  # as even as integers allow


@pytest.mark.parametrize("R,m", [(77, 1), (77, 7), (77, 33), (40, 9), (5, 2), (2**31 - 1, 3)])
@pytest.mark.parametrize("seed,stream", [(0, 0), (1, 5), (2**64 - 1, 2**32 - 1)])
def test_every_index_lies_in_its_stratum(R, m, seed, stream):
    lo, n = mr.strata(R, m)
    idx = mr.indices(R, m, seed, stream)
    assert ((idx >= lo[:-1]) & (idx < lo[:-1] + n)).all()
    assert len(set(idx.tolist())) == m  # without replacement
    assert (idx == mr.indices(R, m, seed, stream)).all()


def test_the_whole_data_set_is_the_identity():
    for R in (1, 6, 77):
        assert (mr.indices(R, R, 12345, 7) == np.arange(R)).all()
        assert (mr.strata(R, R)[1] == 1).all()


def test_streams_and_seeds_give_different_batches():
    a = mr.indices(10**6, 64, 1, 0)
    assert (a != mr.indices(10**6, 64, 1, 1)).any() and (a != mr.indices(10**6, 64, 2, 0)).any()


def test_row_frequencies_are_uniform_within_five_sigma():
    """R = 8, m = 2, seed 1, streams 0 .. 255: every row is drawn Binomial(256, 1/4) times, sigma = 6.93; 5 sigma = 35"""
    count = np.zeros(8, dtype=np.int64)
    for s in range(256):
        idx = mr.indices(8, 2, 1, s)
        count[idx] += 1
    assert count.sum() == 512 and count[:4].sum() == 256
    assert (np.abs(count - 64) <= 35).all(), count


# ---- the layout tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", mr.KINDS)
def test_segment_table_sums_to_the_packed_buffer(nf, kind):
    for rows in (mr.R_MAIN, 9):
        tgt = mr.build(nf, kind, torch.float64, "cpu", rows=rows)
        segs, wseg, w = nf.flows.minibatch_segments(tgt)
        assert sum(n for _, n in segs) == tgt.p0.numel()
        assert all(n == rows for per_row, n in segs if per_row) and segs[wseg][0]
        assert w == tgt.A.shape[1]
        # the weight segment is where the constructor put the weights: every fifth is 0
        at = sum(n for _, n in segs[:wseg])
        assert (tgt.p0[at:at + rows][::5] == 0).all() and (tgt.p0[at:at + rows][1:5] > 0).all()
        for m in (1, rows - 2):  # the batch's buffer: the per-row segments shrink, nothing else
            assert sum(m if per_row else n for per_row, n in segs) == tgt.p0.numel() - sum(per_row for per_row, _ in segs) * (rows - m)
    if kind == "dglm_negbin":
        tgt = mr.build(nf, kind, torch.float64, "cpu")
        assert tgt.table_len == 4 and nf.flows.minibatch_segments(tgt)[0][-1] == (False, 4)  # cnt | ctab exist


def test_numpy_gather_at_the_full_size_is_the_identity(nf):
    for kind in mr.KINDS:
        tgt = mr.build(nf, kind, torch.float32, "cpu")
        segs, wseg, _ = nf.flows.minibatch_segments(tgt)
        p0, p1 = tgt.p0.numpy(), tgt.A.numpy()
        q0, q1 = mr.gather(p0, p1, segs, wseg, tgt.rows, tgt.rows, np.arange(tgt.rows))
        assert q0.tobytes() == p0.tobytes() and q1.tobytes() == p1.tobytes()


# ---- the constructor -----------------------------------------------------------------------------------------------------------------
def test_constructor_refusals(nf):
    X = torch.randn(64, 3, dtype=torch.float64)
    lab = torch.arange(64) % 2
    unsupported = [nf.DiagGaussTarget(torch.zeros(3), torch.ones(3)), nf.BananaTarget(3, 0.1, 1.0),
                   nf.MvNormalTarget(torch.zeros(3, dtype=torch.float64), torch.eye(3, dtype=torch.float64)),
                   nf.LogisticRegressionTarget(X, lab.double()),
                   nf.OrdinalRegressionTarget(X, lab, 2),
                   nf.ConditionalLogitTarget(X, torch.arange(64) // 4, (torch.arange(64) % 4 == 0))]
    for t in unsupported:
        with pytest.raises(nf.NFHipError, match="row-minibatch"):
            nf.MinibatchTarget(t, 1)
    glm = nf.GLMTarget("logit", X)
    for bad in (0, -1, 65, 2.0, True, None, "3"):
        with pytest.raises(nf.NFHipError, match=r"batch_rows must be an integer in 1\.\.64"):
            nf.MinibatchTarget(glm, bad)
    with pytest.raises(nf.NFHipError, match="seed"):
        nf.MinibatchTarget(glm, 8, seed=-1)
    with pytest.raises(nf.NFHipError, match="device"):  # a host target: the gather is device work
        nf.MinibatchTarget(glm, 8)
    # a non-centring layer reads the groups from the FULL target (the batch's fixed segments are copies of them)
    with pytest.raises(nf.NFHipError, match="HierarchicalGLMTarget"):
        nf.noncentred(None, glm)
    assert nf.MinibatchTarget in nf.objectives._BUILTIN and nf.MinibatchTarget in nf.objectives._LINPRED
    assert "MinibatchTarget" in nf.__all__


# ---- the symbol ----------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound_and_the_abi_is_4(nf):
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    ext = set(re.findall(r"^extern (?:int|int32_t|int64_t)\s+(nf_\w+)\s*\(", hdr, re.M))
    assert ext == set(nf._lib.EXT_SYMBOLS) == {"nf_target_minibatch"}
    assert not set(nf._lib.EXT_SYMBOLS) & set(nf.SYMBOLS) and len(nf.SYMBOLS) == 49
    lib = C.CDLL(nf.LIB_PATH)
    assert hasattr(lib, "nf_target_minibatch")
    fn = nf.load_library().nf_target_minibatch
    assert fn.restype is C.c_int and len(fn.argtypes) == 13
    proto = re.search(r"^extern int nf_target_minibatch\(([^;]*)\);", hdr, re.M | re.S).group(1)
    assert len(proto.split(",")) == 13
    assert nf.load_library().nf_abi_version() == 4 and int(re.search(r"#define NF_ABI_VERSION (\d+)", hdr).group(1)) == 4
    assert [f[0] for f in nf._lib.Target._fields_] == ["kind", "p0", "p1", "s0", "s1"]
    jl = open(os.path.join(ROOT, "ext", "NormalizingFlowsNFHipExt.jl")).read()
    assert ":nf_target_minibatch" in jl


def test_argument_errors_come_before_any_device_work(nf):
    """NF_ERR_ARG (-1) and NF_ERR_UNSUPPORTED (-2) with a stand-in context and HOST buffers: nothing may be touched"""
    from normalizingflows_jl_amd._lib import Target

    lib = nf.load_library()
    ctx = C.cast((C.c_char * 4096)(), C.c_void_p)
    src = (C.c_double * 4096)()
    dst0, dst1 = (C.c_double * 4096)(), (C.c_double * 4096)()
    p, q0, q1 = (C.cast(b, C.c_void_p).value for b in (src, dst0, dst1))
    R, d = 77, 6

    def call(t, d=d, elems=d + 2 * R + 2, m=7, o0=q0, o1=q1, out=True, dtype=1, ctx=ctx):
        res = Target(-7, 0, 0, -1.0, -1.0)
        code = lib.nf_target_minibatch(ctx, dtype, C.byref(t) if t is not None else None, d, elems, m, 1, 0, None, None, C.c_void_p(o0),
                                       C.c_void_p(o1), C.byref(res) if out else None)
        assert (res.kind, res.p0, res.p1, res.s0, res.s1) == (-7, None, None, -1.0, -1.0)  # no error leaves a descriptor behind
        return code

    glm = lambda k=9, s0=float(R), s1=1.0: Target(k, p, p + 8 * 2048, s0, s1)
    for dtype in (0, 1):
        for kind, s0, s1, dd in ((0, 0.0, 0.0, d), (1, 0.1, 1.0, d), (2, 0.0, 3.0, d), (3, 1.0, 1.0, 2), (4, 2.0, 0.2, 2), (5, 0.0, 0.0, d),
                                 (6, float(R), 1.0, d), (8, 3.0, 0.0, d), (32, 64.0, 3.0, d), (33, 64.0, 1.0, d)):
            assert call(glm(kind, s0, s1), d=dd, dtype=dtype) == -2, kind
        for kind in (7, 14, 21, 27, 28, 34, -1):  # unassigned kinds
            assert call(glm(kind), dtype=dtype) == -1, kind
        assert call(None, dtype=dtype) == -1
        assert call(glm(), out=False, dtype=dtype) == -1
        assert call(glm(), o0=0, dtype=dtype) == -1 and call(glm(), o1=0, dtype=dtype) == -1
        assert call(Target(9, 0, p, float(R), 1.0), dtype=dtype) == -1 and call(Target(9, p, 0, float(R), 1.0), dtype=dtype) == -1
        assert call(glm(), m=0, dtype=dtype) == -1 and call(glm(), m=-3, dtype=dtype) == -1 and call(glm(), m=R + 1, dtype=dtype) == -1
        assert call(glm(), o0=p, dtype=dtype) == -1 and call(glm(), o1=p + 8 * 2048, dtype=dtype) == -1          # aliased outputs
        for elems in (0, d + 2 * R + 1, d + 2 * R + 3, d + 3 * R + 2):
            assert call(glm(), elems=elems, dtype=dtype) == -1, elems                                            # not the kind's layout
        assert call(glm(), ctx=None, dtype=dtype) == -1
    assert call(glm(), dtype=2) == -1
    # the other layouts' element counts: one element off is refused (G = 2; C = 2; H = 1)
    p_h, p_d = d - 2, d - 3
    fits = {16: (d + 2 * R + 2 + 3 * p_h + 4 * 2 + 1, 2.0), 29: (d + 2 * R + 4 + 3 * p_d + 4 * 3, 2.0), 15: (2 * R + 2, 2.0), 22: (3 * R + 4, 1.0)}
    for kind, (elems, s1) in fits.items():
        dd = 5 if kind == 22 else d  # H = 1: d = p + 2
        for off in (-1, 1):
            assert call(glm(kind, float(R), s1), d=dd, elems=elems + off) == -1, (kind, off)
    nb = d + 3 * R + 4 + 3 * p_d + 4 * 3  # NEGBIN: the table length is what p0_elems leaves, 0 .. 4096
    assert call(glm(31, float(R), 2.0), elems=nb - 1) == -1 and call(glm(31, float(R), 2.0), elems=nb + 4097) == -1
    assert bytes(dst0) == bytes(8 * 4096) and bytes(dst1) == bytes(8 * 4096) and bytes(src) == bytes(8 * 4096)


# ---- resources and sources -----------------------------------------------------------------------------------------------------------
def test_gather_kernels_use_no_scratch(nf):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    rows = kernel_resources.kernel_table(os.path.join(ROOT, "normalizingflows.jl_amd", "build"))
    assert len(rows) > 200, "the objects' metadata notes were not readable"
    hit = [r for r in rows if r[0].startswith("void k_minibatch_gather<")]
    assert len(hit) == 2, [r[0][:60] for r in hit]  # float, double
    for name, agpr, vgpr, sgpr, scratch, lds in hit:
        assert scratch == 0 and agpr == 0, (name, scratch, agpr)
        assert vgpr <= 64, (name, vgpr)   # a copy kernel: full occupancy
        assert lds == 64, (name, lds)     # the workgroup's sixteen row indices


def test_the_new_source_is_built_and_has_no_build_time_variants():
    assert "nf_minibatch.hip" in SOURCES
    src = open(os.path.join(ROOT, "normalizingflows.jl_amd", "csrc", "nf_minibatch.hip")).read()
    assert not re.search(r"^\s*#\s*if(def|ndef)?\b.*\bNF_", src, re.M)
    assert "atomic" not in src.replace("no atomics", "")
