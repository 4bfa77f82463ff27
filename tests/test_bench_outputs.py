"""bench.py's plain run and its --dump-outputs: a plain run times the K steps and reports them, nothing else; the dump holds
what the timed path handed its caller after the last timed step, the same in every run with the same arguments, so that two
builds can be compared output for output.  --full keeps the extra figures (roofline, per-kernel table, sustained clock)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from __graft_entry__ import ROOT

torch = pytest.importorskip("torch")


def _bench_module():
    spec = importlib.util.spec_from_file_location("nf_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_stays_under_its_limit_with_a_fixed_sample(tmp_path):
    """cfg 4's parameter count with --split-calls (theta, both moments and the gradient) is more than the limit: every array
    is cut to its share by the same seeded sample in every run; arrays that fit are written whole."""
    b = _bench_module()
    rng = np.random.default_rng(3)
    P = 4214784
    arrays = {k: rng.standard_normal(P).astype(np.float32) for k in ("theta", "adam_m", "adam_v", "grad")}
    arrays["loss"] = np.array([1.5], dtype=np.float64)
    arrays["grad_norm"] = np.array([2.5], dtype=np.float64)
    b.dump_outputs(str(tmp_path / "a"), arrays)
    b.dump_outputs(str(tmp_path / "b"), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(k + ".npy" for k in arrays)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64_000_000
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == arrays[f[:-4]].dtype and np.array_equal(x, y), f
    assert 0 < np.load(tmp_path / "a" / "theta.npy").size < P
    assert np.isin(np.load(tmp_path / "a" / "theta.npy"), arrays["theta"]).all()
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == 1.5
    small = {"theta": arrays["theta"][:1000]}
    b.dump_outputs(str(tmp_path / "c"), small)
    assert np.array_equal(np.load(tmp_path / "c" / "theta.npy"), small["theta"])


def test_bench_refuses_zero_timed_steps():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--steps" in p.stderr


def _run(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "NF_BENCH_ONE_DEVICE")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_plain_run_is_lean_and_its_dump_is_the_last_timed_step(tmp_path):
    common = ["--steps", "3", "--warmup", "2", "--batch", "4096"]
    a = _run(common + ["--dump-outputs", str(tmp_path / "a")])
    b = _run(common + ["--dump-outputs", str(tmp_path / "b")])
    for rec in (a, b):
        assert rec["steps"] == 3 and rec["warmup"] == 2 and rec["ms_per_step"] > 0
        assert rec["value"] == pytest.approx(4096 / (rec["ms_per_step"] * 1e-3), rel=1e-6)
        assert (rec["metric"], rec["unit"], rec["higher_is_better"], rec["dtype"]) == ("elbo_samples_per_sec", "samples/s", True, "f32")
        assert not {"roofline", "kernels", "cpu_baseline"} & set(rec)
        assert rec["ms_per_step_sustained_clock"] is None
    da, db = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(da) == {"theta", "adam_m", "adam_v", "loss", "grad_norm"}
    P = a["config"]["params"]
    for k in ("theta", "adam_m", "adam_v"):
        assert da[k].dtype == np.float32 and da[k].shape == (P,) and np.all(np.isfinite(da[k])), k
    assert float(da["loss"][0]) == a["config"]["final_loss"]
    assert float(da["grad_norm"][0]) == a["config"]["final_gradient_norm"]
    for k in da:  # same arguments, same inputs: the same bits (tools/stress_determinism.py holds the kernels to that)
        assert np.array_equal(da[k], db[k]), k
    # --full measures more AFTER the timed steps (pre-warm, bracketed steps): its dump is still the last timed step
    f = _run(common + ["--full", "--no-cpu-baseline", "--prewarm", "2", "--dump-outputs", str(tmp_path / "f")])
    assert {"roofline", "kernels"} <= set(f) and f["ms_per_step_sustained_clock"] is not None
    df = _load(tmp_path / "f")
    for k in da:
        assert np.array_equal(da[k], df[k]), k
