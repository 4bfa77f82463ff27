"""RealNVP parity off the Glorot-initialisation regime, on every kernel path and under the arithmetic switches (`-m gpu`).

Every other RealNVP parity test runs at init_params (Glorot weights, all biases exactly zero) plus at most 0.05 of noise, on N(0, 1)
inputs: every tanh argument O(1), s well inside (-1, 1), no hidden unit deep in the leaky arm for the whole batch, no bias above
0.2, no input above ~ 4 -- where a kernel that reads the t net's bias for the s net's, loses a bias of the zero-padded rows, takes
1 - s^2 from the wrong register near saturation, clamps nf_tanh at the wrong place or accumulates the six-term bf16 products in
an order that only holds for operands of one magnitude is almost invisible.  The cases of tests/affine_cases.py prescribe the
scale outputs (saturated both ways, on the three sides of nf_tanh's clamp, linear, zero; gain = 0: the same for every sample,
gain = 1: sample-dependent on top), conditioner biases of several units, hidden units at -3, +3 and exactly 0, and inputs of
scale 0.3 ... 4 with an all-zero, a +-30, a 1e-20 and a 1e3 / 1e-3 column; tests/test_affine_cases_cpu.py holds the cases to the
conditions that keep the float32-oracle floor from licensing a wrong kernel and every gradient check at the plain GRAD_RTOL.

Per case, against the float64 oracle through tests/parity.py (float32: floor = the float32 oracle; Float64: F64_RTOL / F64_GRAD,
no floor): forward y and ladj on the value set, each coupling's conditioner rows bit for bit; inverse x and ladj on the forward
image against o.flow_inv (not a round trip); nf_layer_apply chained against the whole map bit for bit; ELBO loss and gradient on
the gradient set (supplied draws; on the NetGeo shapes also under nf_ctx_set_stash_budget(1 << 32) and (0): the stashed and the
recompute pass), with in-library draws (diagonal Gaussian, and Banana where the target forward is fused), the pullback
nf_flow_fwd_keep + nf_flow_bwd_kept, nf_elbo_step against the split calls where it is fused, forward-KL loss and gradient.  The
shapes are the smallest that reach each implementation (affine_cases.SHAPES, checked against geo_size / nf_deep_geo_id,
nf_wide_supported / wide_fits_mid, l64_ok and g64m_geo: none had to move), and the launches are checked by their profiler names.
The kernels behind environment switches (read once per process) run the same checks in a child process each.

The exact-zero pre-activation.  The reverse kernels of nf_coupling.hip, nf_deep.hip, nf_wide.hip and nf_rqs.hip took the
leaky-ReLU slope from the SIGN BIT of the activation (nf_sign_mask16), so a pre-activation of exactly +0 -- a unit with zero weights
and bias, or every unit of a fresh flow on a conditioner half of exactly 0 -- was differentiated with slope 1 where the reference
(ifelse(x > 0, x, 0.01x)) and this library's own nf_generic64.hip / nf_g64m.h use 0.01: db and dW rows 100 x the reference's.
affine_cases.ZERO_CASES give three first-layer units of both nets of both couplings zero rows and a zero bias;
test_exact_zero_preactivations_take_the_leaky_slope holds the ELBO gradient (supplied and in-library draws) to GRAD_RTOL and reports
the twelve bias entries on their own.  nf_sign_mask16 now builds the mask from the sign of 0 - v (set exactly when v > 0) and
inverts it, so +-0 count as slope 0.01 in every kernel that shares it, fused and split forms alike -- with ONE exception: the
hidden-64 stashing forward whose masks k_affine_bwd_pair reads (bench.py's step) keeps the sign bit, because the exact rule
made that step 1.8 % slower than the parent, more than the parent's own spread (PAIR_COST below; DESIGN sections 4 and 5), and
exactly those passes of f32_d64_h64 (default and stashed; the recompute pass is asserted) are a strict xfail.  bench.py --workload cfg3 (nf_rqs.hip, fixed): 1.0430 / 1.0413 /
1.0425 ms against the parent's 1.0401 / 1.0389 / 1.0400.

What else the cases found.  Every parity criterion holds on every shape, gain and switch row (float32 gradients within 6.4e-6 of
|g|inf against GRAD_RTOL = 1e-4, Float64 ones within 4e-15; the table of tests/parity.py, `affine regimes:`).  nf_layer_apply
chained was NOT the whole map bit for bit on the two LDS-resident float32 families (another arithmetic for the single coupling,
another summation order of ladj); it is now -- see test_layer_apply_chained_equals_the_whole_map_bit_for_bit.
"""
import json
import os
import subprocess
import sys

import pytest

import affine_cases as A
import parity as P
from __graft_entry__ import ROOT, load_package

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


@pytest.mark.parametrize("gain", [0, 1])
@pytest.mark.parametrize("shape", list(A.SHAPES))
def test_affine_regimes_against_oracle(nf, shape, gain):
    chk = A.device_checks(nf, A.case(shape, gain), A.parts_of(shape, layer=False))
    assert not chk.failed, "\n".join(chk.failed)


@pytest.mark.parametrize("gain", [0, 1])
@pytest.mark.parametrize("shape", list(A.SHAPES))
def test_layer_apply_chained_equals_the_whole_map_bit_for_bit(nf, shape, gain):
    """nf_layer_apply of each coupling, chained, against nf_flow_fwd on the value set: y and ladj bit for bit (the distance is
    recorded in the parity table as `nf_layer_apply chained against the whole map`).

    What it found on the two LDS-resident float32 families, in units of the plain element-wise tolerance, gain 0 / 1:
      NetGeo shapes: y differed -- d = 6: 0.86 / 0.50, d = 64: 1.96 / 1.96, d = 63: 1.32 / 1.32 -- and so did ladj at gain = 1
        (0.35, 3.17, 2.53).  nf_flow_fwd ran k_affine_chain, whose GEMMs are six-term bf16 products, nf_layer_apply ran
        k_affine_apply on fp32 MFMAs: two arithmetic variants, each within tolerance of the oracle, but a composition of the
        bijectors that was not the flow.  nf_layer_apply now runs k_affine_apply_b6, the chain's own coupling_step on the same
        bf16-triple images; under NF_FWD_FP32 both run that function on fp32 MFMAs (k_affine_apply calls coupling_step too), and the
        fwd_fp32 switch row holds this criterion as well.
      ladj, NetGeo and nf_deep.hip shapes (0.01 ... 0.12 of the tolerance, a last bit): the chain kernels kept ONE running per-lane
        sum of s over all couplings and folded the two half-waves once at the end, a single coupling folds its own sum.  The forms
        that store ladj now fold per coupling (the fused training forwards keep the running sum).  One ulp was left at hidden 64:
        hipcc contracted nf_tanh's last product into the sum in one kernel and not in the other; coupling_step's sum is now
        compiled without contraction.
    The wide, l64 and Float64 shapes always passed: there the whole map IS the per-coupling launches."""
    chk = A.device_checks(nf, A.case(shape, gain), ("layer",))
    assert not chk.failed, "\n".join(chk.failed)


@pytest.mark.parametrize("shape", list(A.SHAPES))
def test_affine_regime_shapes_land_on_their_kernels(nf, shape):
    """one forward and one ELBO gradient of each shape: the family's launches ran, by profiler name, and no other family's"""
    ran = A.dispatch(nf, A.case(shape, 1))
    assert A.family_ok(ran, A.FAMILY[shape]), f"{shape}: expected {A.FAMILY[shape]}, launches {ran}"


# The one path left on the sign-bit rule (nf_coupling.hip, stash_mask16): the hidden-64 stashing forward behind k_affine_bwd_pair.
PAIR_COST = ("the exact mask costs the hidden-64 stashing forward + k_affine_bwd_pair step 0.5558 / 0.5596 / 0.5617 ms against the parent's "
             "0.5517 / 0.5484 / 0.5478 (three alternating runs of bench.py on one MI355X: +1.8 %, the parent's own spread 0.7 %), so that "
             "forward keeps the sign-bit mask: +0 differentiates with slope 1 there (default and stashed pass; the recompute pass is exact)")


# (shape, passes): the hidden-64 shape is split so that only the passes that read the stashing forward's masks carry the xfail
ZERO_RUNS = [(s, "all") for s in A.ZERO_SHAPES if s != "f32_d64_h64"] + [
    pytest.param("f32_d64_h64", "default+stashed", marks=pytest.mark.xfail(strict=True, reason=PAIR_COST)), ("f32_d64_h64", "recompute")]
ZERO_PARTS = {"all": ("elbo", "elbo_rng"), "default+stashed": ("elbo_default", "elbo_stashed", "elbo_rng"), "recompute": ("elbo_recompute",)}


@pytest.mark.parametrize("shape,passes", ZERO_RUNS)
def test_exact_zero_preactivations_take_the_leaky_slope(nf, shape, passes):
    """Three first-layer units of both nets of both couplings with zero rows and a zero bias (affine_cases.ZERO_CASES): the ELBO
    gradient from supplied draws (on the NetGeo shapes also the stashed and the recompute pass) and from in-library draws at
    GRAD_RTOL; the twelve bias entries are reported on their own (`zero-unit bias entries`).  Before the change of nf_sign_mask16
    the four sign-mask shapes (d = 6, 64, 16 x 3 hidden, 70) returned those entries 100 x the reference's.  At d = 64 the default and
    the stashed pass (and the in-library draws, which take the default) are the strict xfail; the recompute pass under
    nf_ctx_set_stash_budget(0), the way round that DESIGN and INTEGRATION.md name, is asserted by itself -- and once more under
    NF_AFFINE_NO_STASH in the switch rows."""
    chk = A.device_checks(nf, A.case(shape, 1, True), ZERO_PARTS[passes])
    assert not chk.failed, "\n".join(chk.failed)


SWITCHES = ("NF_AFFINE_NO_STASH", "NF_BWD_NO_PAIR", "NF_BWD_ONE_WAVE_B6", "NF_BWD_FP32", "NF_BWD_DW_FP32", "NF_FWD_FP32", "NF_FWD_B6_STASH",
            "NF_STASH_SLIM", "NF_WIDE_FP32", "NF_DEEP_OFF", "NF_G64_NO_F64_MFMA")
CFG2 = "f32_d64_h64"  # d = 64, hidden (64, 64): bench.py's shape, where the stash / pair / B6 switches select their kernels


def _items(shape, parts, family=None):
    return [{"shape": shape, "gain": g, "zero": False, "parts": list(parts), "family": family or A.FAMILY[shape]} for g in (0, 1)]


def _zero_item(shape, parts):
    return [{"shape": shape, "gain": 1, "zero": True, "parts": list(parts), "family": A.FAMILY[shape]}]


# row -> (switches set, items); `family`: where the shape lands with the switch set
ROWS = {
    "affine_no_stash": (("NF_AFFINE_NO_STASH",), _items(CFG2, ("elbo", "elbo_rng", "tape")) + _zero_item(CFG2, ("elbo_default", "elbo_rng"))),
    "bwd_no_pair": (("NF_BWD_NO_PAIR",), _items(CFG2, ("elbo", "tape"))),
    "bwd_no_pair_one_wave_b6": (("NF_BWD_NO_PAIR", "NF_BWD_ONE_WAVE_B6"), _items(CFG2, ("elbo", "tape"))),
    "bwd_fp32": (("NF_BWD_FP32",), _items(CFG2, ("elbo",))),
    "bwd_dw_fp32": (("NF_BWD_DW_FP32",), _items(CFG2, ("elbo",))),
    "fwd_fp32": (("NF_FWD_FP32",), _items(CFG2, ("fwd", "inv", "layer", "elbo_rng", "step")) + _items("f32_d6_h32", ("fwd", "inv", "layer", "elbo_rng", "step"))),
    "fwd_b6_stash": (("NF_FWD_B6_STASH",), _items(CFG2, ("fwd", "elbo_rng", "step"))),
    "stash_slim": (("NF_STASH_SLIM",), _items(CFG2, ("elbo", "elbo_rng"))),
    "wide_fp32": (("NF_WIDE_FP32",), _items("f32_d70_h40x96", ("fwd", "inv", "elbo", "fkl"))),
    "deep_off": (("NF_DEEP_OFF",), _items("f32_d16_h64x3", A.parts_of("f32_d16_h64x3"), "l64") + _items("f32_d16_h24", A.parts_of("f32_d16_h24"), "l64")),
    "g64_no_f64_mfma": (("NF_G64_NO_F64_MFMA",), _items("f64_d8_h16", A.parts_of("f64_d8_h16"), "g64")),
}

_CHILD = r"""
import json, os, sys
root = os.environ["NF_ROOT"]
for p in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
    sys.path.insert(0, p)
from __graft_entry__ import load_package
import parity as P, affine_cases as A
nf = load_package()
job = json.loads(os.environ["NF_AFFINE_JOB"])
chk = A.Checks()
ran = []
for it in job["items"]:
    c = A.case(it["shape"], it["gain"], it["zero"])
    A.device_checks(nf, c, tuple(it["parts"]), chk, job["tag"])
    ran.append(A.dispatch(nf, c))
print(json.dumps({"measured": P.MEASURED, "failed": chk.failed, "ran": ran}))
"""


@pytest.mark.parametrize("row", list(ROWS))
def test_affine_regimes_under_environment_switches(row):
    """Each arithmetic variant behind a switch, in a process of its own (the switches are read once per process): the child runs the
    checks above at the default path's tolerances and prints one JSON line -- every measured ratio, the criteria of tests/parity.py
    that did not hold and the launches of each item by profiler name; the parent records the ratios and asserts that none failed
    and that each shape landed on the family the switch sends it to."""
    names, items = ROWS[row]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update({k: "1" for k in names})
    env.update(NF_ROOT=ROOT, NF_AFFINE_JOB=json.dumps({"tag": "[" + " ".join(k + "=1" for k in names) + "] ", "items": items}))
    p = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert r["measured"] and all(k.startswith("affine regimes: [") for k in r["measured"])
    for k, v in r["measured"].items():
        P.record(k, v)
    assert not r["failed"], "\n".join(r["failed"])
    for it, ran in zip(items, r["ran"]):
        assert A.family_ok(ran, it["family"]), f"{it['shape']}: expected {it['family']}, launches {ran}"
