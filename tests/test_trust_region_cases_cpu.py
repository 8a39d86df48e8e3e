"""The case table of tests/trust_region_cases.py is what it says, on the oracle alone (no GPU).

Per case: the window's trace is the recorded one; every rho is at least RHO_MARGIN from 0.1, 0.25 and 0.75; a
NEGCURVTURE exit has d_Hd <= -NEGCURV_MARGIN |delta| |H delta|; the kinds (clip, all-rejected, shrink, give-up) have the
shape the device test relies on.  These are conditions on the INPUTS: a case that misses one is replaced by another,
never kept with a looser assertion on the device side.  Then the census: the table as a whole holds every
(solve path, branch) pair tests/test_trust_region_branches_gpu.py is there for, so that a later edit of the table cannot
quietly drop one.
"""
import numpy as np
import pytest

import trust_region_cases as C
from trust_region_cases import (ACC, ADD1, ADD2, BEGIN_END, CASES, DEVICE, DR, EXCR, HI, LINEAR, LO, MANY, MID, MULTI, NEGC,
                                ONE, POLL, REJ, SYM, SYM_HOST, VCYCLE)


def case_d(case):
    return {"random": case.problem[1], "lattice": 2, "grid": 3}.get(case.problem[0]) or (2 if "kitti" in case.problem[1] else 3)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_window_is_the_recorded_one(oracle, case):
    X0, radius, oo, Xo = C.run_window(oracle, case)
    trace = oo.result.trace
    assert C.observed(oracle, trace) == case.expect
    assert oo.result.outer_iters == len(case.expect)
    for t in trace:
        assert min(abs(t["rho"] - th) for th in (0.1, 0.25, 0.75)) >= C.RHO_MARGIN, t["rho"]
        assert t["accept"] == (t["rho"] > 0.1)  # the tiny-decrease clause decides nowhere in the table
        if oracle.TCG_NAMES[t["status"]] == NEGC:
            row = t["tcg"][-1]
            assert row["d_Hd"] <= -C.NEGCURV_MARGIN * row["norm_d"] * row["norm_Hd"], row
    deltas = [t["Delta_in"] for t in trace] + [trace[-1]["Delta"]]
    if case.kind == "clip":  # Delta, 2 Delta, 4 Delta, then 5 Delta (= Delta_max) instead of 8 Delta, and one step with it
        assert case.expect[:3] == ((EXCR, HI, ACC),) * 3 and len(case.expect) >= 4
        assert deltas[:4] == [radius, 2 * radius, 4 * radius, 5 * radius]
    elif case.kind == "all-rejected":
        assert all(e[2] == REJ for e in case.expect) and len(case.expect) >= 2
        assert np.array_equal(Xo, X0) and oo.result.fOpt == oo.result.fInit
    elif case.kind == "shrink":  # RTR_iterations == 1: every try restarts from the input with a quarter of the radius
        assert len(case.expect) in (3, 4, 5) and [e[2] for e in case.expect] == [REJ] * (len(case.expect) - 1) + [ACC]
        assert [t["Delta_in"] for t in trace] == [radius / 4 ** k for k in range(len(trace))]
        assert not np.array_equal(Xo, X0)
    elif case.kind == "give-up":
        assert len(case.expect) == 12 and all(e[2] == REJ for e in case.expect)  # QuadraticOptimizer.cpp:80-99
        assert np.array_equal(Xo, X0)
    else:
        assert case.kind == "window" and 2 <= len(case.expect) <= 3
        for a, b in zip(trace[:-1], trace[1:]):  # a rejection is followed by a run from the same point, radius / 4
            if not a["accept"]:
                assert b["x"] is a["x"] and b["Delta_in"] == 0.25 * a["Delta_in"]
    if case.precond == "multilevel":
        # the V-cycle's dense coarse level goes through BLAS: the window must not depend on how BLAS threads split it
        from threadpoolctl import threadpool_limits
        with threadpool_limits(1):
            one = C.run_window(oracle, case)[2].result
        assert (one.tcg_iters, one.outer_iters, C.observed(oracle, one.trace)) == (oo.result.tcg_iters, oo.result.outer_iters,
                                                                                 case.expect)


def branches(case):
    """The branches a case's window takes (what the census counts)."""
    e, out = case.expect, set()
    if case.kind in ("shrink", "give-up"):
        return {"shrink loop: accepted after several tries" if case.kind == "shrink" else "shrink loop: twelve tries, gives up"}
    for k, (exit_, band, decision) in enumerate(e):
        if decision == REJ:
            out.add("rejection after " + exit_)
            out.add("rejection at (d, r) = (%d, %d)" % (case_d(case), case.r))
            if k + 1 < len(e):
                out.add("rejection followed by another iteration")
                if e[k + 1][2] == REJ:
                    out.add("two rejections in a row")
        else:
            out.add("accepted, " + band)
            if exit_ == NEGC and band == HI and k + 1 < len(e):
                out.add("radius doubled after NEGCURVTURE, then another iteration")
        if exit_ == NEGC:
            out.add("NEGCURVTURE exit")
    if case.kind == "clip":
        out.add("radius clipped at Delta_max")
    if case.kind == "all-rejected":
        out.add("all steps rejected")
    elif any(x[2] == REJ for x in e) and any(x[2] == ACC for x in e):
        out.add("mixed window")
    out.add("a case with d = %d" % case_d(case))
    return out


FULL = (["rejection after " + NEGC, "rejection after " + EXCR, "accepted, " + LO, "accepted, " + MID, "accepted, " + HI,
         "two rejections in a row", "radius doubled after NEGCURVTURE, then another iteration",
         "radius clipped at Delta_max", "all steps rejected"] +
        ["rejection at (d, r) = (%d, %d)" % dr for dr in DR])
REQUIRED = {MULTI: FULL + ["shrink loop: accepted after several tries", "shrink loop: twelve tries, gives up"],
            ONE: FULL,
            POLL: ["rejection followed by another iteration", "a case with d = 2", "a case with d = 3"]}
for _path in (ADD1, ADD2, VCYCLE, SYM, SYM_HOST, LINEAR):
    REQUIRED[_path] = ["rejection followed by another iteration", "NEGCURVTURE exit"]
REQUIRED[LINEAR] = REQUIRED[LINEAR] + ["a case with d = 2", "a case with d = 3"]
for _path in (DEVICE, BEGIN_END, MANY):
    REQUIRED[_path] = ["rejection followed by another iteration", "NEGCURVTURE exit", "all steps rejected", "mixed window"]


def census(cases):
    """{(path, branch)} the table misses."""
    have = {(p, b) for c in cases for p in c.paths for b in branches(c)}
    return sorted((p, b) for p, bs in REQUIRED.items() for b in bs if (p, b) not in have)


def test_census_every_path_keeps_every_branch():
    assert len({c.name for c in CASES}) == len(CASES)
    assert all(set(c.paths) <= set(REQUIRED) and c.paths for c in CASES)
    assert census(CASES) == []
    # and the census notices: without the cases of any one (path, branch) pair, it names that pair
    for path, bs in REQUIRED.items():
        for b in bs:
            rest = [c for c in CASES if not (path in c.paths and b in branches(c))]
            assert (path, b) in census(rest), (path, b)
