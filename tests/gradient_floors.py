"""Oracle-side helpers of the gradient checks that more than one test module needs (plain module: numpy and the oracle only).

min_abs_preact: how close a sample comes to a leaky-ReLU kink.  fp32_recompute_floor / fp32_recompute_kink_floor /
recompute_bound / KINK_CAP: what a reverse pass by invertible recompute may be off by (tests/test_gpu_parity.py,
tests/test_gpu_cotangent_carry.py, tests/affine_cases.py).
"""
import numpy as np

import nf_oracle as o
import parity as P


def min_abs_preact(spec, th, xs, skip_first_layer=()):
    """per sample, the smallest |pre-activation| of any leaky-ReLU unit in the oracle's forward pass; `skip_first_layer`: units
    of every net's first hidden layer left out (units that sit on the kink by construction)"""
    _, _, states = o.flow_fwd(spec, th, xs, keep=True)
    out = np.full(xs.shape[1], np.inf)
    for li, x in zip(reversed(o.layers_flat_order(spec)), states):
        for net in li.nets:
            _, acts = o.mlp_forward(th, net, x[li.idx_c], None, keep=True)
            for l, a in enumerate(acts[1:-1]):  # a = leakyrelu(z): z = a for a > 0, a / 0.01 otherwise
                z = np.abs(np.where(a > 0, a, a / 0.01))
                if l == 0 and len(skip_first_layer):
                    z = np.delete(z, list(skip_first_layer), axis=0)
                out = np.minimum(out, z.min(axis=0))
    return out


def fp32_recompute_floor(spec, th64, otgt, xs64, jitter_seed=None):
    """The float32 oracle's gradient with every layer input RECONSTRUCTED by inverting the chain from its output in
    float32 -- what an invertible-recompute reverse pass (k_affine_bwd_all) differentiates.  Its distance from the float64
    gradient grows with depth like the float32 round-trip error of the flow; the stashed pass does not have that term.
    `jitter_seed`: the forward's output moved by N(0, 2^-24) relative first -- a forward that rounds its last bit
    differently (another summation order, fp32 MFMA chain vs six-term bf16 product, truncating vs rounding split)."""
    th32, xs32 = P.f32(th64, xs64)
    t32 = P.f32(otgt)
    n = xs32.shape[1]
    y32, _ = o.flow_fwd(spec, th32, xs32)
    if jitter_seed is not None:
        z = np.random.default_rng(jitter_seed).standard_normal(y32.shape).astype(np.float32)
        y32 = (y32 * (np.float32(1) + np.float32(2.0 ** -24) * z)).astype(np.float32)
    order = list(reversed(o.layers_flat_order(spec)))
    rec, cur = [None] * (len(order) + 1), y32
    rec[len(order)] = y32
    for i in range(len(order) - 1, -1, -1):
        cur, _ = o._layer_inv(spec, th32, order[i], cur)
        rec[i] = cur
    ybar = (-o.target_grad(t32, y32) / n).astype(np.float32)
    lbar = np.full(n, -1.0 / n, dtype=np.float32)
    return o.flow_bwd(spec, th32, rec, ybar, lbar)[1]


def fp32_recompute_kink_floor(spec, th64, otgt, xs64, gref, nseeds=12):
    """Worst gradient error (max abs / |g|inf) of the float32 reconstruct-by-inversion oracle over `nseeds` last-bit jitters
    of the forward output.  The error of an invertible-recompute reverse pass is not a smooth function of the forward's
    rounding: a hidden unit within the reconstruction error (2e-5 ... 9e-5) of its leaky-ReLU kink takes the other slope,
    a jump of |delta a| / n per (sample, unit).  On the d = 64, 8-coupling case below the SAME numpy code lands on 1e-6,
    2.2e-4 or 9e-3 of |g|inf depending on the jitter seed (measured, round 5) -- the device's own roundings pick one of those
    outcomes, which one changes with every change of the forward's arithmetic (round 4's truncating split: 3.3e-4; round
    5's rounding split: 3.0e-3; fp32 MFMAs: 3.1e-4).  So the recompute tests bound the device by this measured
    distribution instead of a constant."""
    scale = float(np.abs(gref).max())
    errs = [float(np.abs(fp32_recompute_floor(spec, th64, otgt, xs64, s) - gref).max() / scale) for s in [None] + list(range(nseeds))]
    return max(errs), errs[0]


KINK_CAP = 1e-2  # no jitter outlier may license more than this: a recompute gradient off by > 1 % of |g|inf is wrong


def recompute_bound(kink):
    """The asserted bound of an invertible-recompute gradient: the stated tolerance, or CFLOOR x the measured kink floor, but
    never more than KINK_CAP of |g|inf."""
    return max(P.GRAD_RTOL, min(P.CFLOOR * kink, KINK_CAP))
