"""The partial-sum regions and the state slots of the multi-launch solve (dpgo_amd/csrc/handoff.h): tests/cxx/test_handoff.cpp
compiled with the host compiler against that header alone -- no HIP, no library."""
import os
import subprocess

from conftest import ROOT


def test_partial_regions_and_state_slots(tmp_path):
    exe = os.path.join(str(tmp_path), "test_handoff")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "dpgo_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "test_handoff.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "handoff: ok" in p.stdout, p.stdout + p.stderr
