"""Built-in target parity off the N(0, 1) cloud, at every evaluation site (`-m gpu`).

The log-densities and scores of DiagGauss, Banana, Funnel, WarpedGauss and Cross are written once (target_term, nf_targets.h) and
instantiated at eight sites, each with its own gather of y0, y1 and Funnel's s2 and its own padding mask.  The cases of
tests/target_cases.py put the samples where these densities are hard (exp(-y0) from 2e-9 to 1.6e5, Cross on ridges 0.02 wide and
40 sigma out, WarpedGauss at r = 1e-6 and across atan2's branch cut, b y0^2 in the hundreds, variances eight decades apart), at
d = 2, 3 and on both sides of every template boundary, with n = 1, 33 and 77; tests/test_target_cases_cpu.py holds them to the
conditions under which a float32 kernel can be held to the plain tolerance WITHOUT a floor on the conditioned elements.

  site 1      k_target<float / double>: nf.target_logp with its gradient on the cloud itself -- every target, parameter set, d, n;
              and once more behind every simple flow's forward (nf.batched_elbos)
  site 2      k_target_tiled behind a near-identity RealNVP flow and a near-identity full-rank flow, the cloud as supplied draws
  site 3      k_simple_apply's fused target: the training forward of planar / radial flows beyond k_simple_step's register budget
              (5 and 13 layers, Float64 d = 129), followed by simple_bwd.  nf.batched_elbos of a simple flow does NOT use it: it runs
              k_simple_apply without the target and then k_target -- site 1 once more, behind every simple flow of the table
  site 4      k_simple_step: mean-field, Float64, d > 64, radial d < 8; its two switch arms in a child process each
  sites 5, 6  k_planar_step / k_radial_step: Float32 planar / radial at d <= 64
  sites 7, 8  k_affine_chain_tgt / k_rqs_chain_tgt (DiagGauss: the chain kernels' own code) on in-library draws that the flow carries
              to the cloud; nf_elbo_value_and_grad, one nf_elbo_step, and site 1 on the same y against the fused loss
Per case of sites 2-6, loss and gradient of nf.value_and_gradient against o.neg_elbo_value_and_grad where target_cases.aggregate_ok,
and the per-sample terms of nf.batched_elbos against o.batched_elbos under target_cases.hold -- which is a per-sample check of
site 2 only: behind a simple flow the terms come from k_target.  SITES 3, 4, 5 AND 6 ARE HELD BY LOSS AND GRADIENT ALONE (their
entry points return nothing per sample), sites 7 and 8 by loss, gradient, one step and the cross-site sum.  Every case asserts by
profiler name that the intended kernel ran and no sibling.  The figures go to the parity table under `target regimes:`, keyed by
the launches that produced them, the worst of each (flow, dtype, target, d) group; tools/target_regimes_summary.py reduces them to
profiles/target_regimes_parity_measured.json.

Measured, worst over flows, d, parameter sets, clouds and n (the target that sets it in brackets), device / float32 oracle:
  per sample -- conditioned elements in units of the plain tolerance, then max |err| / |ref|inf
    site 1, k_target<float>: log p                       0.71 / 0.25 (Funnel)   2.4e-6 / 1.4e-6 (WarpedGauss)
    site 1, k_target<float>: score                       0.72 / 0.25 (Funnel)   3.8e-6 / 4.1e-6 (WarpedGauss / Cross)
    site 1, k_target<double>, of 1e-12 + 1e-10 |ref|     5.7e-4                 9.2e-15
    site 2, k_target_tiled: ELBO terms                   0.64 / 0.25 (Funnel)   6.3e-5 / 9.9e-6 (Banana; by its largest term 2.4e-7 / 3.0e-7)
    k_target behind a simple flow's forward: ELBO terms  0.59 / 0.25 (Banana)   6.1e-5 / 9.9e-6 (Banana; 2.7e-7 / 5.5e-7); Float64 1.4e-4, 1.5e-13
  loss (relative) and gradient (of |g|inf)
    site 2, target_tiled behind RealNVP / full-rank      4.2e-6 / 9.9e-7 (WarpedGauss)   7.4e-6 / 7.4e-6 (DiagGauss)
    site 3, simple_apply + simple_bwd                    2.5e-6 / 9.9e-7 (Funnel)        7.8e-6 / 8.5e-6; Float64 3.8e-15, 1.4e-14
    site 4, simple_step                                  3.0e-6 / 9.7e-7 (WarpedGauss)   9.9e-6 / 9.9e-6; Float64 3.1e-15, 1.2e-14
    site 4 under NF_PLANAR_NO_MFMA / NF_RADIAL_NO_LANE   1.6e-6 / 9.5e-7 (Funnel)        9.5e-6 / 9.6e-6
    site 5, planar_step                                  1.7e-6 / 9.9e-7 (Banana)        8.1e-6 / 8.1e-6 (DiagGauss)
    site 6, radial_step                                  3.2e-6 / 9.4e-7 (Funnel)        1.3e-5 / 9.6e-6 (Funnel)
    site 7, affine_chain_tgt (DiagGauss: affine_chain)   1.5e-6 / 9.7e-7                 7.2e-6 / 7.2e-6; one step the same; site 1 on the same y 0.07 of its bound
    site 8, rqs_chain_tgt (DiagGauss: rqs_chain)         1.2e-6 / 8.0e-7                 2.0e-5 / 9.5e-6 (Funnel); site 1 on the same y 0.014 of its bound
No site was wrong.  What the cases found: o.cross_logp / o.cross_grad evaluated float32 points in float64 (a float64 component table),
so every float32 floor of a Cross check was a float64 figure -- at the origin of Cross(5, 0.02) it read 0.11 x the tolerance where
the device and a real float32 evaluation read 5 x (fixed in oracle/nf_oracle.py; the cloud is norm-wise only now); and a planar
"near-identity" with |w| = 0.03 that carried y0 from -11.4 to -7.4 (target_cases.flow_theta).
Sensitivity, on scratch builds: y1 read from sample 0 in k_target turned 7 of these tests red (site 1 Banana, Cross and WarpedGauss in
both dtypes, and the mean-field flow whose batched_elbos runs k_target); y1 read from lane 0 in nf_target_epilogue.h turned 13 red
(sites 7 and 8: Banana at every d, Cross and WarpedGauss, behind both chain kernels; Funnel and DiagGauss do not read y1 and
stayed green, as did site 2).  The `i >= 0` perturbation of an s2 sum was not demonstrated.
"""
import json
import os
import subprocess
import sys

import pytest

import parity as P
import target_cases as T
from __graft_entry__ import ROOT, load_package

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nf():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return load_package()


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("target", T.TARGETS)
def test_site1_target_logp_and_score(nf, target, f64):
    """k_target on the cloud itself: per-sample log p and score, every parameter set, every d of target_cases.dims_of, n = 1, 33, 77"""
    chk = T.Checks()
    for pi in range(len(T.PARAMS[target])):
        for d in T.dims_of(target):
            T.site1(nf, target, pi, d, f64, chk)
    assert not chk.failed, f"{len(chk.failed)} failures:\n" + "\n".join(chk.failed[:40])


def test_site1_runs_the_standard_layout_kernel(nf):
    tgt = T.device_target(nf, torch, "funnel", 0, 9, torch.float32)
    y = T._cm(torch, T.points("funnel", 0, 9, 0), torch.float32)
    ran = T.launched(nf, nf._lib.context_for(y.device), lambda: nf.target_logp(tgt, y, with_grad=True))
    assert T.only(ran, target=1) and not ran["layout_convert"], ran


FLOW_IDS = [(kind, f64, nl, d) for kind, f64, nl, dims in T.FLOW_CASES for d in dims]


def _assert_flow(chk, counts, what):
    assert not chk.failed, f"{what}: {len(chk.failed)} failures:\n" + "\n".join(chk.failed[:40])
    for target, (nl, ng, nall) in counts.items():  # (decided from the oracles alone: the aggregate checks are not vacuous)
        assert T.eligible_enough(nl, ng, nall), f"{what} {target}: {nl} losses and {ng} gradients of {nall} cases were eligible"


@pytest.mark.parametrize("kind,f64,nl,d", FLOW_IDS, ids=[f"{k}-{'f64' if f else 'f32'}-{'x' + str(nl) + '-' if nl else ''}d{d}" for k, f, nl, d in FLOW_IDS])
def test_sites_2_to_6_supplied_draws(nf, kind, f64, nl, d):
    """the cloud as supplied draws of the family's near-identity flow.  Site 2 (realnvp, fullrank): per-sample ELBO terms, loss and
    gradient.  Sites 3 / 4 / 5 / 6 (value_and_gradient of the simple flows, by target_cases.train_launch): loss and gradient only --
    their entry points return nothing per sample, and nf.batched_elbos of a simple flow is k_target (site 1) behind its forward"""
    chk, counts = T.flow_site(nf, kind, f64, d, nl)
    _assert_flow(chk, counts, f"{kind} d={d}")


_CHILD = r"""
import json, os, sys
root = os.environ["NF_ROOT"]
for p in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
    sys.path.insert(0, p)
from __graft_entry__ import load_package
import parity as P, target_cases as T
nf = load_package()
job = json.loads(os.environ["NF_TARGET_JOB"])
chk, counts = T.Checks(), {}
for d in job["dims"]:
    _, c = T.flow_site(nf, job["kind"], False, d, None, chk, job["tag"], no_tile=True)
    counts[str(d)] = c
print(json.dumps({"measured": P.MEASURED, "failed": chk.failed, "counts": counts}))
"""


@pytest.mark.parametrize("switch", list(T.SWITCH_ROWS))
def test_site4_switch_arms(switch):
    """k_simple_step<float> at d <= 64, which only NF_PLANAR_NO_MFMA / NF_RADIAL_NO_LANE reach (read once per process): the same cases in
    a child process, launches asserted by name there"""
    kind, dims = T.SWITCH_ROWS[switch]
    env = {k: v for k, v in os.environ.items() if k not in T.SWITCH_ROWS}
    env.update({switch: "1", "NF_ROOT": ROOT, "NF_TARGET_JOB": json.dumps({"kind": kind, "dims": list(dims), "tag": f"[{switch}=1] "})})
    p = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert r["measured"] and all(k.startswith("target regimes: [") for k in r["measured"])
    for k, v in r["measured"].items():
        P.record(k, v)
    assert not r["failed"], f"{len(r['failed'])} failures:\n" + "\n".join(r["failed"][:40])
    for d, counts in r["counts"].items():
        for target, (nl, ng, nall) in counts.items():
            assert T.eligible_enough(nl, ng, nall), (switch, d, target, nl, ng, nall)


PLACED = [(kind, target, d) for kind in ("realnvp", "nsf") for d in T.PLACED_DIMS[kind] for target in T.targets_at(d)]


@pytest.mark.parametrize("kind,target,d", PLACED, ids=[f"{k}-{t}-d{d}" for k, t, d in PLACED])
def test_sites_7_8_in_library_draws(nf, kind, target, d):
    """k_affine_chain_tgt / k_rqs_chain_tgt (and the chain kernels' own diagonal-Gaussian code, TGT == 0, on the wide-variance case):
    the flow places the cloud (target_cases.placed_theta; which clouds are reachable: the module docstring there), loss and gradient
    of nf_elbo_value_and_grad(xs = NULL) and of one nf_elbo_step against the oracle on the regenerated draws, and site 1 on the same
    y against the fused loss."""
    chk, (nl, ng, nall) = T.placed_site(nf, kind, target, d)
    assert not chk.failed, f"{len(chk.failed)} failures:\n" + "\n".join(chk.failed[:40])
    # (at least one each, not a share as at sites 2-6: the draws are the device sampler's, within 3e-6 of the oracle's, and a case at the
    # edge of aggregate_ok may fall either way)
    assert nl >= 1 and ng >= 1, f"{nl} losses and {ng} gradients of {nall} cases were eligible"
