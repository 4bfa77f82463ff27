"""CPU checks of the forward-KL training step's C ABI (nf_loglikelihood_step, nf_loglikelihood_step_enqueue): declared in
the header, bound in _lib.SYMBOLS with the header's arity, exported by libnfhip.so, and argument errors caught before any
device work."""
import ctypes as C
import os
import re

import pytest

from __graft_entry__ import ROOT, build, load_package

NAMES = ("nf_loglikelihood_step", "nf_loglikelihood_step_enqueue")


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


def _header_arity(name):
    hdr = open(os.path.join(ROOT, "include", "nfhip.h")).read()
    m = re.search(rf"^int\s+{name}\s*\(([^)]*)\)\s*;", hdr, re.M)
    assert m, f"{name} is not declared in include/nfhip.h"
    return len([p for p in m.group(1).split(",") if p.strip()])


@pytest.mark.parametrize("name", NAMES)
def test_symbols_are_declared_bound_and_exported_with_matching_arity(nf, name):
    assert name in nf.SYMBOLS
    restype, argtypes = nf.SYMBOLS[name]
    assert restype is C.c_int
    assert len(argtypes) == _header_arity(name)
    assert hasattr(C.CDLL(nf.LIB_PATH), name)
    assert nf.load_library().nf_abi_version() == 4


def _desc():
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc

    desc = FlowDesc()
    desc.kind, desc.dtype, desc.d, desc.nlayers, desc.n_hidden = NF_KIND["realnvp"], 0, 64, 4, 2
    desc.hdims[0] = desc.hdims[1] = 64
    return desc


def test_null_pointers_and_negative_sizes_are_argument_errors(nf):
    """NF_ERR_ARG (-1) for a NULL context, theta or ys and for N_local < 0 -- returned before the context is touched, so
    a stand-in context pointer is enough here."""
    lib = nf.load_library()
    desc = _desc()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    ctx = C.cast((C.c_char * 64)(), C.c_void_p)
    counter = C.cast((C.c_uint32 * 1)(), C.c_void_p)

    def step(ctx_, theta, ys, n):
        return lib.nf_loglikelihood_step(ctx_, C.byref(desc), theta, p, p, ys, n, 0, 0, 1e-3, 0.9, 0.999, 1e-8, None, None)

    def enqueue(ctx_, theta, ys, n, cnt=counter):
        return lib.nf_loglikelihood_step_enqueue(ctx_, C.byref(desc), theta, p, p, ys, n, 0, cnt, 1e-3, 0.9, 0.999, 1e-8, None)

    for call in (step, enqueue):
        assert call(None, p, p, 16) == -1
        assert call(ctx, None, p, 16) == -1
        assert call(ctx, p, None, 16) == -1
        assert call(ctx, p, p, -1) == -1
    assert enqueue(ctx, p, p, 16, cnt=None) == -1


# the forward-KL chain kernels: k_affine_chain<G, INVERSE, FUSED, STASH, ...> and k_rqs_chain<G, INVERSE, FUSED, ...> with
# INVERSE and FUSED both set (demangled names, as tools/kernel_resources.py prints them)
FKL_KERNELS = (
    "void k_affine_chain<NetGeo<1, 1, 1, 1, 4>, true, true, true, false, false>(",
    "void k_affine_chain<NetGeo<1, 2, 2, 1, 4>, true, true, true, false, false>(",
    "void k_rqs_chain<RqsGeo<1, 1, 1, 8, 4, 2>, true, true, true>(",
    "void k_rqs_chain<RqsGeo<1, 1, 1, 8, 4, 2>, true, true, false>(",
    "void k_rqs_chain<RqsGeo<1, 1, 1, 10, 2, 2>, true, true, false>(",
)


def test_forward_kl_chain_kernels_use_no_scratch(nf):
    """Every forward-KL chain instantiation is built, register-resident (no private segment) and fits the 256 registers of
    two waves per SIMD; the K = 10, d <= 32 spline geometry (whose chain kernels spill) has none."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources

    rows = kernel_resources.kernel_table(os.path.join(ROOT, "normalizingflows.jl_amd", "build"))
    for prefix in FKL_KERNELS:
        hit = [r for r in rows if r[0].startswith(prefix)]
        assert len(hit) == 1, f"{prefix} is not in the built objects"
        name, _agpr, vgpr, _sgpr, scratch, _lds = hit[0]
        assert scratch == 0 and vgpr <= 256, (name[:100], vgpr, scratch)
    assert not [r for r in rows if r[0].startswith("void k_rqs_chain<RqsGeo<1, 1, 1, 10, 4, 2>, true, true,")]
