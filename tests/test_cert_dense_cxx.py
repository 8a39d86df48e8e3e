"""The host algebra of the certificate's eigen-solver (dpgo_amd/csrc/cert_dense.h / cert_dense.cpp):
tests/cxx/test_cert_dense.cpp compiled with the host compiler and the address and undefined-behaviour sanitizers against
that file alone -- no HIP, no library."""
import os
import subprocess

from conftest import ROOT


def test_factorizations_assembly_and_every_step_of_the_eigen_solver(tmp_path):
    exe = os.path.join(str(tmp_path), "test_cert_dense")
    csrc = os.path.join(ROOT, "dpgo_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "cxx", "test_cert_dense.cpp"), os.path.join(csrc, "cert_dense.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "cert_dense: ok" in p.stdout, p.stdout + p.stderr
