"""CPU checks of the Hamiltonian flow's host side: the reverse kernels (k_hf_bwd, k_hf_bwd_inv) keep one gradient row of
P = 4D + 3Dn elements in dynamic LDS, the launch paths opt in to 128 KiB of it, and nf_hf_supported refuses a descriptor
whose row is larger -- check_desc answers NF_ERR_UNSUPPORTED before any device work, so a stand-in context is enough."""
import ctypes as C

import pytest

from __graft_entry__ import build, load_package

NF_ERR_UNSUPPORTED = -2


@pytest.fixture(scope="module")
def nf():
    build()  # no-op when libnfhip.so is up to date
    return load_package()


def _standin():
    return C.cast((C.c_char * 4096)(), C.c_void_p)


def _tape_bytes(nf, dtype, d, n, L=1, kind=0, N=70):
    from normalizingflows_jl_amd._lib import NF_KIND, FlowDesc, Target

    lib = nf.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    score = Target(kind, p, p, 1.0, 1.0)
    desc = FlowDesc()
    desc.kind, desc.dtype, desc.d, desc.nlayers, desc.K = NF_KIND["hamiltonian"], dtype, d, n, L
    desc.score = C.cast(C.pointer(score), C.c_void_p)
    lib.nf_tape_bytes.restype = C.c_int64
    assert int(lib.nf_param_count(C.byref(desc))) == 2 * d + 3 * (d // 2) * n
    return int(lib.nf_tape_bytes(_standin(), C.byref(desc), N))


@pytest.mark.parametrize("dtype,n,P,ok", [(1, 169, 16352, True), (1, 170, 16448, False), (1, 171, 16544, False),
                                          (0, 340, 32768, True), (0, 341, 32864, False)])
def test_lds_gradient_row_is_bounded_on_the_host(nf, dtype, n, P, ok):
    """d = 64 (D = 32), diagonal-Gaussian score: the largest row that fits 128 KiB is P = 16 384 in Float64 and 32 768 in
    Float32; one block more is refused by every entry point (here: nf_tape_bytes) with NF_ERR_UNSUPPORTED."""
    assert 4 * 32 + 3 * 32 * n == P
    es = 8 if dtype == 1 else 4
    assert (P * es <= 128 * 1024) == ok
    got = _tape_bytes(nf, dtype, 64, n)
    if ok:
        assert got >= 70 * 64 * es  # TAPE_X: the flow input
    else:
        assert got == NF_ERR_UNSUPPORTED


def test_row_bound_is_about_the_row_not_the_block_count(nf):
    """The same block counts at a small D stay supported, and the older limits still answer first."""
    assert _tape_bytes(nf, 1, 4, 341) >= 0       # P = 8 + 6 * 341
    assert 8 + 6 * 2730 == 16388 and _tape_bytes(nf, 1, 4, 2730) == NF_ERR_UNSUPPORTED
    assert 8 + 6 * 2729 == 16382 and _tape_bytes(nf, 1, 4, 2729) >= 0
    assert _tape_bytes(nf, 1, 66, 1) == NF_ERR_UNSUPPORTED   # D = 33 > HF_MAXD
    assert _tape_bytes(nf, 1, 64, 1, L=17) == NF_ERR_UNSUPPORTED  # L > HF_MAXL
    assert _tape_bytes(nf, 1, 2, 1, kind=1) == NF_ERR_UNSUPPORTED  # Banana needs D >= 2
    assert _tape_bytes(nf, 1, 2, 1, kind=0) >= 0                   # D = 1: the diagonal Gaussian only
