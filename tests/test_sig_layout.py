"""wasmedge_amd/csrc/sig_layout.h: how a signature's values lie in cells, slots and the device
tables of the device-resident calls -- the one definition every staging and result path of the
library uses (staging.cpp, hostcall.cpp, the global accessors). The header is plain C++, so its
contract with args_io.hip and calls_io.hip is checked here without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wasmedge_amd", "csrc")


def test_layout_under_sanitizers(tmp_path):
    """tests/c/sig_layout_check.cpp: layouts, pack and unpack maps, the value codec, the per-name
    table and the per-module result table against literals written out by hand from the formats,
    under the address and undefined-behaviour sanitizers. No report, no differing word."""
    exe = str(tmp_path / "sig_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "sig_layout_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
