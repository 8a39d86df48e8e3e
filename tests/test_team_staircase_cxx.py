"""evalTeam and escapeTeam of the C++17 mirror (include/dpgo_hip.hpp): tests/cxx/test_team_escape.cpp compiled with the host
compiler against libdpgo_hip.so, as tests/test_team_certificate_cxx.py builds its program."""
import os
import subprocess

import pytest

from conftest import ROOT


def _build(tmp_path):
    exe = os.path.join(str(tmp_path), "test_team_escape")
    libdir = os.path.join(ROOT, "dpgo_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cxx", "test_team_escape.cpp"), "-L", libdir, "-ldpgo_hip",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_cxx_team_escape_compiles_and_refuses_without_device(tmp_path):
    import dpgo_amd
    exe = _build(tmp_path)
    if dpgo_amd.device_count() == 0:  # (with a device the gpu test below runs the program)
        p = subprocess.run([exe], capture_output=True, text=True)
        assert p.returncode == 77, p.stdout + p.stderr


@pytest.mark.gpu
def test_cxx_team_escape_twisted_ring(tmp_path):
    exe = _build(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "team escape: ok" in p.stdout, p.stdout + p.stderr
