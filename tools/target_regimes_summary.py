#!/usr/bin/env python3
"""Reduce the `target regimes:` rows of a parity table (tests/test_gpu_target_regimes.py; conftest.py dumps the table at the end of a
`-m gpu` session) to the worst figure per (what ran, dtype, target, array, measure), over flows, d, parameter sets, clouds and n.

    python tools/target_regimes_summary.py PARITY.json [OUT.json]     (OUT: profiles/target_regimes_parity_measured.json)

The rows are keyed by the launches that produced them, as the tests assert them by profiler name:
  nf_target_logp: k_target                               site 1, per-sample log p and score
  batched_elbos: target_tiled                            site 2, per-sample ELBO terms behind a RealNVP / full-rank flow
  batched_elbos: simple_apply, then k_target             site 1 behind a simple flow's forward -- NOT sites 3-6
  value_and_gradient: target_tiled | split | simple_step | planar_step | radial_step     sites 2, 3, 4, 5, 6: loss and gradient only
  in-library draws: affine_chain_tgt | affine_chain | rqs_chain_tgt | rqs_chain          sites 7, 8: loss, gradient, one step, site 1 on the same y
"""
import json
import re
import sys

TARGETS = ("funnel", "banana", "cross", "warped", "diaggauss")


def ran_of(key):
    """(what ran, dtype) of a `target regimes:` row"""
    dt = "f64" if " f64" in key.split(":")[1] + key.split(":")[2] else "f32"
    sw = re.search(r"\[(NF_[A-Z_]+)=1\]", key)
    tag = f" [{sw.group(1)}=1]" if sw else ""
    if "site 1 " in key:
        return "nf_target_logp: k_target", dt
    m = re.search(r"in-library draws \((\w+)\)", key)
    if m:
        return "in-library draws: " + m.group(1), dt
    m = re.search(r"\((batched_elbos|value_and_gradient): ([^)]*)\)", key)
    return f"{m.group(1)}: {m.group(2)}{tag}", dt


def reduce(table):
    out = {}
    for key, v in table.items():
        if not key.startswith("target regimes:"):
            continue
        ran, dt = ran_of(key)
        target = next(t for t in TARGETS if f" {t} d=" in key)
        array = re.search(r" d=\d+: ([^\[]*) \[", key).group(1)
        k = f"target regimes: {ran}: {dt}: {target}: {array} {key[key.rindex('['):]}"
        out[k] = max(out.get(k, 0.0), v)
    return dict(sorted(out.items()))


if __name__ == "__main__":
    red = reduce(json.load(open(sys.argv[1])))
    with open(sys.argv[2] if len(sys.argv) > 2 else "profiles/target_regimes_parity_measured.json", "w") as f:
        json.dump(red, f, indent=1)
        f.write("\n")
    print(f"{len(red)} rows")
