"""CPU-side check of the fused planar / radial / mean-field ELBO step's routing and workspace layout: the host side of every
translation unit of libnfhip.so is built with `hipcc --offload-host-only -fsanitize=address,undefined` (as
tests/test_sanitizers.py builds it) and tests/host/nf_simple_step_host_check.hip drives step_fusable_simple and SimpleStepBufs
through it with a hand-made context -- no device, no launch.  Per flow (planar d = 64 x 10 f32, planar d = 2 x 10 f64, radial
d = 5 x 10 f32, mean-field d = 4 f64, planar d = 200 x 30 f32), N in {1, 15, 16, 17, 1000, 65 536} and stash budgets {-1, 0, 3 MiB}:
the predicate is true for the first four flows and false for the last, false with a communicator, a general base or a target
that fails its check; the layout plus the arena's tails fits nf_workspace_bytes and the intermediates bound, is no larger
than the split form's, and its buffers are 256-byte aligned and disjoint."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from __graft_entry__ import CSRC, HIPCC, ROOT, SOURCES

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def test_simple_step_routing_and_layout_under_asan_ubsan(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    flags = ["--offload-host-only", *SAN, "-std=c++17", "-Wno-unused-value", "-Wno-comment", "-Wno-unused-result"]

    def cc(src, obj):
        r = subprocess.run([HIPCC, *flags, "-c", src, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, (src, r.stderr[-3000:])
        return obj

    jobs = [(os.path.join(CSRC, s), str(tmp_path / s.replace(".hip", ".o"))) for s in SOURCES if s != "nf_api.hip"]
    jobs.append((os.path.join(ROOT, "tests", "host", "nf_simple_step_host_check.hip"), str(tmp_path / "check.o")))  # includes nf_api.hip
    with ThreadPoolExecutor(max_workers=4) as ex:
        objs = list(ex.map(lambda j: cc(*j), jobs))
    # no HIP runtime is linked: every HIP symbol gets a stand-in that reports hipErrorNoDevice, the device binaries are empty
    und = subprocess.run(["nm", "-u", *objs], capture_output=True, text=True).stdout.split()
    syms = sorted({t for t in und if t.startswith("hip") or t.startswith("__hip")})
    stub = ['#include <cstdio>', 'extern "C" {']
    for t in syms:
        if t.startswith("__hip_fatbin_"):
            stub.append(f"char {t}[64] = {{0}};")
        elif t == "__hipRegisterFatBinary":
            stub.append("void **__hipRegisterFatBinary(void *) { static void *h[1]; return h; }")
        elif t in ("__hipRegisterFunction", "__hipUnregisterFatBinary", "__hipRegisterVar", "__hipRegisterManagedVar"):
            stub.append(f"void {t}(...) {{}}")
        elif t == "hipGetErrorString":
            stub.append('const char *hipGetErrorString(int) { return "hip stand-in: no device"; }')
        else:
            stub.append(f"int {t}(...) {{ return 100; }}")
    stub.append("}")
    stub_src = tmp_path / "hip_standins.cpp"
    stub_src.write_text("\n".join(stub) + "\n")
    stub_obj = str(tmp_path / "hip_standins.o")
    r = subprocess.run(["g++", "-c", str(stub_src), "-o", stub_obj], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    exe = str(tmp_path / "nf_simple_step_host_check")
    clangxx = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "clang++")
    r = subprocess.run([clangxx, *SAN, "-o", exe, *objs, stub_obj, "-ldl", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "nf_simple_step host check: ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
