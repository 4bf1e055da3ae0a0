"""Memory-error check of the host JPEG entropy decoder (deconv_api_amd/csrc/jpeg_dec.cpp), the part of the
GPU decode path that parses untrusted request bytes. A stand-alone program (tests/native/jpeg_dec_stress.cpp,
its own main) is built with AddressSanitizer + UBSan from the parser and the project's encoder, and feeds the
parser every truncation of a stream and 6000 fixed-seed mutations on exact-size heap buffers. The program is
run directly; nothing is loaded into Python and LD_PRELOAD is left alone."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deconv_api_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "native", "jpeg_dec_stress.cpp"), os.path.join(CSRC, "jpeg_dec.cpp"),
       os.path.join(CSRC, "jpeg_enc.cpp")]


def test_jpeg_parser_address_ub_sanitizer(tmp_path):
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("LD_PRELOAD is set: the sanitizer runtime would not come first in the process")
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is needed: this is the parser's memory-safety check and must not go missing quietly"
    exe = str(tmp_path / "jpeg_dec_stress")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-pthread", "-DDVJPEG_NO_CLONES", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", f"-I{CSRC}", *SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=20)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    ok, unsupported = (int(x.split("=")[1]) for x in r.stdout.split()[-2:])
    assert ok >= 4 and unsupported >= 1000  # both outcomes were exercised
