"""Every library switch that selects a kernel, a storage or a launch geometry (csrc/options.h, DPGO_OPTIONS) is exercised by
some GPU test: a switch added without one fails here, on a machine without a GPU.  Switches that change only timing or
reporting, or that are covered through another handle of the same choice, are listed below with the reason."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXEMPT = {
    "DPGO_TCG_AHEAD": "how far the host's just-in-time feed runs ahead of the device; launches past the end exit in their "
                      "prologue, so the arithmetic is the same",
    "DPGO_POLL_FIRST": "sleep before the first sweep of the in-kernel all-reduce: timing only",
    "DPGO_POLL_SLEEP": "sleep between sweeps of the in-kernel all-reduce: timing only",
    "DPGO_POLL_FIRST_PAY": "sleep before a payload reduction's first sweep: timing only",
    "DPGO_PERSIST_VERBOSE": "phase report on stderr: reporting only",
    "DPGO_SETUP_TIMING": "set-up section times on stderr: reporting only",
    "DPGO_SETUP_PIN": "placement of host worker threads: timing only",
    "DPGO_PERSIST_MAX_POSES": "size limit of the one-launch solve's selection; both solves are forced by DPGO_PERSIST and "
                              "QuadraticProblem.setPersistent",
    "DPGO_ADDITIVE_TILES": "default of dpgo_problem_additive_tiles, which the two-tile tests set per handle",
    "DPGO_AUTO_COST_RULE": "policy between preconditioners that are tested one by one; the rule itself is tested through "
                           "DPGO_PRECOND_AUTO",
    "DPGO_ML_GRAPH_SIZE": "growth size of the graph aggregates; the hierarchy's shape is mirrored by the oracle through "
                          "setupMultilevel's sizes, the kernels are the same",
}


def _options():
    text = open(os.path.join(ROOT, "dpgo_amd", "csrc", "options.h")).read()
    block = text[text.index("#define DPGO_OPTIONS(X)"):]
    block = block[:block.index("struct Options")]
    names = re.findall(r'X\(\s*\w+\s*,\s*"(DPGO_\w+)"', block)
    assert len(names) == len(set(names)) and len(names) >= 40, names
    return names


def _gpu_test_sources():
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))):
        src = open(path).read()
        if re.search(r"^pytestmark\s*=.*pytest\.mark\.gpu", src, re.M) or "@pytest.mark.gpu" in src:
            out[os.path.basename(path)] = src
    return out


def test_every_geometry_and_kernel_switch_is_named_in_a_gpu_test():
    names = _options()
    sources = _gpu_test_sources()
    assert "test_parity_gpu.py" in sources and "test_launch_geometry_gpu.py" in sources
    untested = [n for n in names if n not in EXEMPT and not any(re.search(r"\b%s\b" % n, s) for s in sources.values())]
    assert not untested, "switches without a GPU test (add one, or an exemption with its reason): %s" % untested


def test_exemptions_name_existing_switches():
    names = set(_options())
    assert not set(EXEMPT) - names, sorted(set(EXEMPT) - names)
    assert all(len(reason) > 20 for reason in EXEMPT.values())
