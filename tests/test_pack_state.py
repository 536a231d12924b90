"""The pack / precision / range protocol that iaf_stack and iaf_conv3x3 share (iaf_amd/csrc/iaf_pack_state.hpp) needs no HIP:
tests/c_abi/iaf_pack_state_walk.cpp includes only that header, walks the protocol -- set_packs, range failures, re-arming,
training, what a prep launch writes, for both kinds of object -- and checks code, packs, f16_off and prepared after every
step.  Built with the address and undefined-behaviour sanitizers and run as a program of its own; no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_abi", "iaf_pack_state_walk.cpp")


def test_pack_state_walk(tmp_path):
    gxx = shutil.which("g++") or shutil.which("c++")
    assert gxx, "no host C++ compiler"
    exe = str(tmp_path / "iaf_pack_state_walk")
    cmd = [gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "iaf_amd", "csrc"), SRC, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, "the walk does not build (the header must compile without HIP):\n" + b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pack state walk ok" in r.stdout


def test_pack_state_header_needs_no_hip():
    """the header includes include/iaf_hip.h and the standard library only"""
    with open(os.path.join(ROOT, "iaf_amd", "csrc", "iaf_pack_state.hpp")) as f:
        incs = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert incs and all(i == '"iaf_hip.h"' or (i.startswith("<") and "hip" not in i) for i in incs), incs
