"""The hierarchy's set-up over index vectors (dpgo_amd/csrc/aggregation.h / aggregation.cpp, taskpool.h, options.h):
tests/cxx/test_aggregation.cpp compiled with the host compiler against those files alone -- no HIP, no library."""
import os
import subprocess

from conftest import ROOT


def test_aggregates_patterns_tables_search_and_shape(tmp_path):
    exe = os.path.join(str(tmp_path), "test_aggregation")
    csrc = os.path.join(ROOT, "dpgo_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", csrc,
                           os.path.join(ROOT, "tests", "cxx", "test_aggregation.cpp"), os.path.join(csrc, "aggregation.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "aggregation: ok" in p.stdout, p.stdout + p.stderr
