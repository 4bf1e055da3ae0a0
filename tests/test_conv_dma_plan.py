"""The LDS-DMA routing policy (deconv_api_amd/csrc/conv_dma_plan.h) on the CPU.

tests/fixtures/conv_dma_routes.txt is a recording of the conv calls of the VGG16 deconvnet, an InceptionV3
and a ResNet-50 DeepDream step and the GPU route tests' shapes on an MI355X, each with the route the binding
reported (tools/record_conv_routes.py). The stand-alone program tests/native/conv_dma_plan_check.cpp,
compiled here with g++ (under AddressSanitizer + UBSan unless LD_PRELOAD is set: a sanitizer runtime must come first
in its process, and the environment is left as it is), replays every row of this family (dma / kw3 / kw3p /
group) through dma_plan() at the recorded CU count and knobs and compares the formatted route; it also
requires one row of every form (tile sizes, split-K, mask, pool_t, KW3P lds / reg / unpool, stream-K, the
tail split, both group configs). No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deconv_api_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "conv_dma_plan_check.cpp")
FIXTURE = os.path.join(ROOT, "tests", "fixtures", "conv_dma_routes.txt")


def _hip_include():
    roots = [r for r in (os.environ.get("ROCM_PATH"), "/opt/rocm") if r]
    found = [r for r in roots if os.path.exists(os.path.join(r, "include", "hip", "hip_runtime_api.h"))]
    assert found, f"HIP headers not found under {roots} (kernels.h includes hip_runtime_api.h)"
    return os.path.join(found[0], "include")


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ not available"
    # with LD_PRELOAD set the sanitizer runtime would not come first: plain build, the route comparison still runs
    san = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                                                   "-fno-sanitize-recover=all"]
    exe = str(tmp_path_factory.mktemp("plan") / "conv_dma_plan_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", *san, "-D__HIP_PLATFORM_AMD__=1", f"-I{_hip_include()}", f"-I{CSRC}",
           SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(exe, path):
    return subprocess.run([exe, path], capture_output=True, text=True, timeout=120)


def test_planner_reproduces_recorded_routes(plan_check):
    r = _run(plan_check, FIXTURE)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    assert "mismatches=0" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    checked = int(r.stdout.split("checked=")[1].split()[0])
    assert checked >= 100, r.stdout


def test_planner_check_detects_a_changed_route(plan_check, tmp_path):
    """The check is live: a recording with one route altered fails on exactly that row."""
    lines = open(FIXTURE).read().splitlines()
    i = next(n for n, ln in enumerate(lines) if ln.endswith("| dma 128x128 st2 ks1"))
    lines[i] = lines[i][: -len("dma 128x128 st2 ks1")] + "dma 256x128 st3 ks1"
    bad = tmp_path / "routes.txt"
    bad.write_text("\n".join(lines) + "\n")
    r = _run(plan_check, str(bad))
    assert r.returncode == 1 and "mismatches=1" in r.stdout and f"line {i + 1}:" in r.stderr, r.stdout + r.stderr
