"""CPU checks of the fused ELBO forward for the Banana, Funnel, WarpedGauss and Cross targets: the new chain kernels
(k_affine_chain_tgt, k_rqs_chain_tgt) are built for every LDS-resident geometry, register-resident (no private segment) and
within the register file of their launch bounds; the C ABI is what it was (no new symbol, version 4)."""
import ctypes as C
import os
import re
import sys

import pytest

from __graft_entry__ import ROOT, build, load_package


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


@pytest.fixture(scope="module")
def table(nf):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    rows = kernel_resources.kernel_table(os.path.join(ROOT, "normalizingflows.jl_amd", "build"))
    assert len(rows) > 200, "the objects' metadata notes were not readable"
    return rows


H32, H64 = "NetGeo<1, 1, 1, 1, 4>", "NetGeo<1, 2, 2, 1, 4>"
RQ8, RQ10, RQ10L = "RqsGeo<1, 1, 1, 8, 4, 2>", "RqsGeo<1, 1, 1, 10, 2, 2>", "RqsGeo<1, 1, 1, 10, 4, 2>"
# k_affine_chain_tgt<G, STASH, SLIM, B6, NW>: with the activation stash on fp32 MFMAs (the training step's default) and
# without a stash on six-term products (nf_elbo_batch_rng, the stash-free gradient), for both geometries
AFFINE = [f"void k_affine_chain_tgt<{g}, {v}, " for g in (H32, H64) for v in ("true, false, false", "false, false, true")]
# k_rqs_chain_tgt<G, B6, TGT, NW>: every spline geometry; K = 8 also with the six-term output layer (its default)
RQS = [f"void k_rqs_chain_tgt<{g}, false, " for g in (RQ8, RQ10, RQ10L)] + [f"void k_rqs_chain_tgt<{RQ8}, true, "]
# TGT is a set of kinds (nf_targets.h: Banana 1, Funnel 2, WarpedGauss 4, Cross 8); every geometry serves all four
ALL_KINDS = 15


def _nw(name):
    """wavefronts per workgroup: the last template argument of both kernels"""
    m = re.search(r", (\d+)>\(", name)
    assert m, name
    return int(m.group(1))


def test_target_chain_kernels_exist_for_every_resident_geometry(table):
    for prefix in AFFINE:
        assert [r for r in table if r[0].startswith(prefix)], f"no kernel named {prefix!r} in the built objects"
    for prefix in RQS:
        hit = [r for r in table if r[0].startswith(prefix)]
        assert hit, f"no kernel named {prefix!r} in the built objects"
        kinds = 0
        for r in hit:
            kinds |= int(re.search(r"(?:true|false), (\d+), \d+>\(", r[0]).group(1))
        assert kinds == ALL_KINDS, (prefix, kinds)


def test_target_chain_kernels_use_no_scratch_and_fit_their_launch_bounds(table):
    """Every instantiation of the two new kernels: 0 bytes of scratch, and registers (accumulation half included) within what
    its __launch_bounds__(64 * NW) leaves a wave: 512 per SIMD lane shared by NW / 4 waves -- 256 at the eight waves of the
    diagonal-Gaussian kernels, 512 where an instantiation was given four."""
    hit = [r for r in table if r[0].startswith("void k_affine_chain_tgt<") or r[0].startswith("void k_rqs_chain_tgt<")]
    assert len(hit) >= len(AFFINE) + len(RQS)
    bad = []
    for name, agpr, vgpr, _sgpr, scratch, _lds in hit:
        nw = _nw(name)
        assert nw in (4, 8), name
        if scratch != 0 or vgpr > 512 // (nw // 4):
            bad.append((name[:110], agpr, vgpr, scratch))
    assert not bad, bad


# every symbol of include/nfhip.h before this change: the fused targets add none
SYMBOLS = """nf_abi_version nf_strerror nf_ctx_create nf_ctx_destroy nf_ctx_set_stream nf_ctx_synchronize nf_workspace_bytes nf_ctx_set_arena
nf_ctx_set_stash_budget nf_param_count nf_layer_count nf_base_sample_logpdf nf_base_logpdf nf_base_rand nf_base_logpdf_general nf_flow_fwd
nf_flow_inv nf_flow_rand nf_layer_apply nf_flow_bwd nf_tape_bytes nf_flow_fwd_keep nf_flow_bwd_kept nf_target_logp nf_elbo_batch
nf_elbo_batch_rng nf_loglikelihood nf_elbo_value_and_grad nf_loglikelihood_value_and_grad nf_adam_update nf_sgd_update nf_elbo_step
nf_ctx_weights_changed nf_ctx_set_weight_cache nf_elbo_step_enqueue nf_loglikelihood_step nf_loglikelihood_step_enqueue
nf_comm_get_unique_id nf_comm_init_rank nf_comm_init_all nf_comm_size nf_ctx_set_comm_bucket_bytes nf_comm_bucket_count
nf_allreduce_grad_loss nf_allreduce_grad_loss_all nf_comm_destroy nf_prof_enable nf_prof_read nf_debug_trace""".split()


def test_abi_is_unchanged(nf):
    assert sorted(nf.SYMBOLS) == sorted(SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t|const char \*)\s*(nf_\w+)\s*\(", hdr, re.M))
    assert declared == set(SYMBOLS), declared ^ set(SYMBOLS)
    lib = nf.load_library()
    assert lib.nf_abi_version() == 4
    for name in SYMBOLS:
        assert hasattr(C.CDLL(nf.LIB_PATH), name)
    assert nf._lib.Target._fields_ == [("kind", C.c_int32), ("p0", C.c_void_p), ("p1", C.c_void_p), ("s0", C.c_double), ("s1", C.c_double)]


def test_graph_form_argument_errors_come_before_any_device_work(nf):
    """nf_elbo_step_enqueue: NF_ERR_ARG (-1) for a NULL context, target, theta or counter and for N < 1, whatever the target
    kind -- returned before the context is touched, so a stand-in context pointer is enough here."""
    from normalizingflows_jl_amd._lib import NF_KIND, NF_TARGET_FUNNEL, FlowDesc, Target

    lib = nf.load_library()
    desc = FlowDesc()
    desc.kind, desc.dtype, desc.d, desc.nlayers, desc.n_hidden, desc.K, desc.B = NF_KIND["nsf"], 0, 9, 2, 2, 10, 5.0
    desc.hdims[0], desc.hdims[1] = 24, 32
    tgt = Target(NF_TARGET_FUNNEL, 0, 0, 0.3, 2.0)
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    ctx = C.cast((C.c_char * 64)(), C.c_void_p)
    cnt = C.cast((C.c_uint32 * 1)(), C.c_void_p)

    def enqueue(ctx_, tgt_, theta, n, counter):
        return lib.nf_elbo_step_enqueue(ctx_, C.byref(desc), tgt_, theta, p, p, n, 5, counter, 1e-3, 0.9, 0.999, 1e-8, None)

    assert enqueue(None, C.byref(tgt), p, 16, cnt) == -1
    assert enqueue(ctx, None, p, 16, cnt) == -1
    assert enqueue(ctx, C.byref(tgt), None, 16, cnt) == -1
    assert enqueue(ctx, C.byref(tgt), p, 0, cnt) == -1
    assert enqueue(ctx, C.byref(tgt), p, 16, None) == -1
