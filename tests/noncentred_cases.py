"""Shapes, targets and inputs shared by test_noncentred_cpu.py and test_gpu_noncentred.py: the hierarchical (d = p + G) and the
dispersion (d = p + G + 1) targets of hier_forms.py / disp_forms.py with the group structure of noncentred_ref.groups, built in
one element type on one device, next to the numpy closed form of the values they hold."""
import numpy as np

import disp_forms as df
import hier_forms as hf
import nf_oracle as o
import noncentred_ref as ncr

ROWS = 33

# name -> (form, p, G): the smallest shapes that reach every path
SHAPES = {
    "small": ("hier", 3, 2),    # one fixed-scale coefficient; groups of sizes 2 and 0
    "disp": ("disp", 3, 2),     # d = p + G + 1: the last coordinate passes through
    "wide": ("hier", 60, 10),   # three feature blocks; the weight-streaming inner RealNVP; fullrank DB = 4
    "pair": ("hier", 56, 8),    # d = 64 under RealNVP [64, 64]: the pair kernel's path
    "nogroup": ("hier", 4, 0),  # G = 0: every coefficient under a fixed scale, S is the identity
}


def dim(shape):
    form, p, G = SHAPES[shape]
    return p + G + (1 if form == "disp" else 0)


def inner_spec(kind, d):
    if kind == "realnvp":
        return o.FlowSpec("realnvp", d, 1, (32, 32))
    if kind == "realnvp64":
        return o.FlowSpec("realnvp", d, 1, (64, 64))
    if kind == "nsf":
        return o.FlowSpec("nsf", d, 1, (32, 32), 8, 30.0)
    assert kind == "fullrank", kind
    return ncr.fullrank_spec(d)


def spec_of(shape, kind, frozen=False):
    form, p, G = SHAPES[shape]
    return ncr.Spec(inner_spec(kind, dim(shape)), ncr.groups(p, G), G, frozen)


def make_target(nf, shape, dtype, device, family=None):
    """(target, ref): the device target and ref(y) -> (log p, score) in y's dtype from the target's own (rounded) arrays"""
    import torch

    form, p, G = SHAPES[shape]
    d = dim(shape)
    grp = np.asarray(ncr.groups(p, G))
    if form == "disp":
        a = df.arrays(family or "normal", d, G, ROWS)
        a["grp"] = grp
        tgt = df.from_arrays(nf, family or "normal", a, G, dtype, device)
        return tgt, df.ref_of(tgt)
    fam = family or "logit"
    a = hf.arrays(fam, d, G, ROWS)
    t = lambda v: torch.tensor(np.asarray(v), dtype=dtype, device=device)
    tgt = nf.HierarchicalGLMTarget(fam, t(a["A"]), torch.tensor(grp, device=device), G, t(a["off"]), t(a["wt"]), t(a["lin"]), const=0.7,
                                   fixed_sigma=a["sig"].tolist(), hyper=a["hyper"], hyper_loc=a["loc"].tolist(),
                                   hyper_scale=a["scl"].tolist())
    return tgt, hf.ref_of(tgt)
