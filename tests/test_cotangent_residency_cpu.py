"""CPU checks that go with the cotangent-resident reverse pass (no GPU): registers and scratch of every two-wave reverse
instantiation, read from the built objects as tests/test_kernel_resources_cpu.py does, and the chunked forward-KL oracle of
tests/oracle_pool.py against the one-call oracle.

The parked cotangents live in the PRODUCER's share of the 256 registers the kernel is allocated for its consumer's sake; a
byte of scratch, or a 257th register, would mean they do not fit there.  Parking changed no kernel's name, so the benchmarked
instantiations stay on test_kernel_resources_cpu.py's lists; this file adds the instantiations those lists do not name (the
fp32 / slim-stash / fp32-dW forms behind the A/B switches, in both directions, whole and ragged batches)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

H64 = "NetGeo<1, 2, 2, 1, 4>"


@pytest.fixture(scope="module")
def table():
    import kernel_resources

    bdir = os.path.join(ROOT, "normalizingflows.jl_amd", "build")
    if not os.path.isdir(bdir) or not any(f.endswith(".o") for f in os.listdir(bdir)):
        import __graft_entry__ as ge

        ge.build()
    rows = kernel_resources.kernel_table(bdir)
    assert len(rows) > 200, "the objects' metadata notes were not readable"
    return rows


def test_every_pair_kernel_instantiation_is_register_resident(table):
    rows = [r for r in table if r[0].startswith(f"void k_affine_bwd_pair<{H64}, ")]
    assert len(rows) == 16, [r[0][:100] for r in rows]  # FULL x INVD x (slim | fp32 | bf16 dX | bf16 dX + dW)
    bad = [(r[0][:100], r[2], r[4]) for r in rows if r[4] != 0 or r[2] > 256]
    assert not bad, f"(name, registers, scratch bytes): {bad}"


def test_stashing_fused_forward_entries_keep_their_resources(table):
    """the y store became a run-time branch (xt == nullptr): the default stashing forward and its target-switch twin stay scratch-free"""
    for prefix in (f"void k_affine_chain<{H64}, false, true, true, false, false>(", f"void k_affine_chain_tgt<{H64}, true, false, false, 8>("):
        hit = [r for r in table if r[0].startswith(prefix)]
        assert hit, prefix
        assert all(r[4] == 0 and r[2] <= 256 for r in hit), [(r[0][:90], r[2], r[4]) for r in hit]


def test_chunked_forward_kl_oracle_equals_the_one_call_oracle():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nf_oracle as o
    import oracle_pool

    spec = o.FlowSpec("realnvp", 6, 1, (8, 8))
    rng = np.random.default_rng(0)
    th = o.init_params(spec, rng) + 0.05 * rng.standard_normal(o.param_count(spec))
    ys = rng.standard_normal((6, 101))
    l0, g0 = o.neg_loglik_value_and_grad(spec, th, ys)
    old = oracle_pool.CHUNK
    try:
        oracle_pool.CHUNK = 17
        l1, g1 = oracle_pool.neg_loglik_value_and_grad(spec, th, ys, workers=2)
    finally:
        oracle_pool.CHUNK = old
    assert abs(l1 - l0) <= 1e-12 * abs(l0)
    assert np.abs(g1 - g0).max() <= 1e-12 * np.abs(g0).max()
