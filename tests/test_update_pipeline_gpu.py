"""k_tcg_update_span's tile pipeline (kernels/tcg.h, PIPE): the multilevel instances request their next tile behind the first
per-piece loop of the tile they are finishing; DPGO_UPDATE_PIPE=0 selects the instances that request it behind the tile's
last store, the order the kernel had before.

Only WHEN a load is issued differs -- the arithmetic, its order and every store are the same -- so the two orders are compared
BIT FOR BIT, iterate and result record, and what can go wrong is the bookkeeping of the two tiles a workgroup now holds at
once (the geometry and the block-Jacobi row of the tile in flight beside those of the tile being finished):

  * every (d, r) the library builds, on every preconditioner path of the multi-launch solve -- the V-cycle with fp32 cycle
    vectors (symmetric storage, the flagship's instance), with DPGO_ML_VECTOR_BITS=64, on the plain storage, block-Jacobi
    and none (the last two run the generic-mode instances, which have no pipelined form: the switch must change nothing);
  * with and without kept directions (DPGO_TCG_DIRS): at 20 and more doubles per pose the instance that also streams eta and
    delta keeps the reference order (kUpdatePipe), below that it is pipelined;
  * 70 and 200 poses: a ragged last wave tile and a ragged last workgroup tile in 2-D and 3-D;
  * launch caps that leave a workgroup one, two and three tiles, and the XCD-eighths walk of 18 tiles on 16 workgroups
    (DPGO_GRID_UPDATE in every test: a launch with one tile per workgroup has nothing to request early and runs the
    reference-order instance, so without a cap these small blocks would not reach the pipelined one);
  * every exit of tCG: the residual test, the boundary step (mode 1 of the kernel: its own per-piece loop), negative
    curvature, the budget.

Blocks: cycle_problem of tests/solve_instance_cases.py (random pose graph, a point near the truth) and sphere2500 from a
random point (tests/trust_region_cases.py) for negative curvature.  No oracle solve: the reference order is the reference.
"""
import numpy as np
import pytest

import solve_instance_cases as SC
import trust_region_cases as TC
from conftest import matrix_to_tiles, tiles_to_matrix, to_product_measurements
from test_launch_geometry_gpu import library_options, tile_poses
from test_tcg_feed_gpu import record

pytestmark = pytest.mark.gpu

REFERENCE = {"DPGO_UPDATE_PIPE": "0"}
KEPT, SUMMED = {}, {"DPGO_TCG_DIRS": "0"}  # (tCG keeps its directions, the default; or sums eta every iteration)
VC32, VC64, VCPLAIN, JACOBI, NONE = "vcycle-fp32-vectors", "vcycle-fp64-vectors", "vcycle-plain", "jacobi", "none"
PATHS = (VC32, VC64, VCPLAIN, JACOBI, NONE)
SYMMETRIC = {"DPGO_SPLIT": "1", "DPGO_SPMM_SYMMETRIC": "1"}  # (what the fp32 copies of the cycle need: host.h, ml_ops32_wanted)
PATH_ENV = {VC32: SYMMETRIC, VC64: dict(SYMMETRIC, DPGO_ML_VECTOR_BITS="64"), VCPLAIN: {}, JACOBI: {}, NONE: {}}


def block(oracle, d, r, n):
    om, _, X, _ = SC.cycle_problem(oracle, SC.Cycle(d, r, 1, SC.GRAPH, n))
    return om, X


def solve(oracle, d, r, n, path, env, om=None, X0=None, **prm):
    """One multi-launch solve on `path` under the switches `env`: (iterate bits, result record, tCG status)."""
    import dpgo_amd
    if om is None:
        om, X0 = block(oracle, d, r, n)
    multilevel = path in (VC32, VC64, VCPLAIN)
    with library_options(dict(PATH_ENV[path], DPGO_PERSIST="0", **env)):
        pg = dpgo_amd.PoseGraph(0, r, d)
        pg.setMeasurements(to_product_measurements(om))
        prob = dpgo_amd.QuadraticProblem(pg)
        prob.setPersistent(False)
        if multilevel:
            info = prob.setupMultilevel()
            assert len(info["sizes"]) == 2, info
        prm.setdefault("gradnorm_tol", 1e-12)
        opt = dpgo_amd.QuadraticOptimizer(prob, dpgo_amd.ROptParameters(precond="multilevel" if multilevel else path, **prm))
        Xg = np.ascontiguousarray(matrix_to_tiles(opt.optimize(tiles_to_matrix(X0)), d))
        rg = opt.getOptResult()
        assert prob.persistentInfo()["last_members"] == 0 and rg.success, rg
        assert not np.isnan(Xg).any()
        span = ((d + 1) * r) % 2 == 0
        if path in (VC32, VC64):  # (the span kernels carry the symmetric storage and with it the fp32 copies)
            bits = prob.multilevelOperatorBits()
            assert (bits["active"], bits["vectors"]) == (span, span and path == VC32), (path, bits)
        assert prob.tcgKernelInfo()["directions"] == (env.get("DPGO_TCG_DIRS") != "0"), (env, prob.tcgKernelInfo())
        del opt, prob
    return Xg.view(np.uint64), record(rg), rg.tCGStatus


def both_orders(oracle, d, r, n, path, env=None, **prm):
    """The solve in the reference order and in the default one: bitwise equal.  Returns the default's (record, status)."""
    env = env or {}
    om, X0 = prm.pop("problem", None) or block(oracle, d, r, n)
    Xr, rr, _ = solve(oracle, d, r, n, path, dict(env, **REFERENCE), om, X0, **prm)
    Xp, rp, status = solve(oracle, d, r, n, path, env, om, X0, **prm)
    what = (d, r, n, path, env, prm, rr, rp)
    assert np.array_equal(Xr, Xp), what
    assert rr == rp, what
    return rp, status


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("d,r", SC.DR)
def test_reference_order_is_bitwise_on_every_instance_and_path(oracle, d, r, path):
    """Every (d, r) x preconditioner path x {kept directions, DPGO_TCG_DIRS=0} on 70 and 200 poses (neither a multiple of a
    wave's 16 / 21 poses nor of the workgroup tile) under an update cap of two workgroups -- a launch whose workgroups hold
    one tile each runs the reference-order instance whatever the switch says (solve.hip, launch_tcg_update), so the cap is
    what puts a second tile into a workgroup: two tiles on two workgroups at 70 poses in 3-D (one in 2-D), four / three
    tiles at 200; two outer iterations of at most six products each."""
    for n in (70, 200):
        assert n % (tile_poses(d, 1) // 4) and n % tile_poses(d, 1)
        for dirs in (KEPT, SUMMED):
            rec, _ = both_orders(oracle, d, r, n, path, dict(dirs, DPGO_GRID_UPDATE="2"), RTR_iterations=2, RTR_tCG_iterations=6)
            assert rec[8] > 0, rec  # (tcg_iterations: the loop ran)


@pytest.mark.parametrize("dirs", [KEPT, SUMMED], ids=["kept", "summed"])
@pytest.mark.parametrize("d,r", [(3, 5), (3, 4), (2, 4)])
def test_one_two_and_three_tiles_per_workgroup(oracle, d, r, dirs):
    """3 P - 7 poses (three workgroup tiles, the last one ragged) under update caps 3, 2 and 1: every workgroup holds one
    tile; workgroup 0 two and workgroup 1 one; one workgroup all three.  17 P + 3 poses under cap 16: the XCD-eighths walk,
    two workgroups of which hold two tiles.  (3, 5): the flagship's instance; (3, 4) and (2, 4): the instances whose
    DPGO_TCG_DIRS=0 form is pipelined too."""
    P = tile_poses(d, 1)
    for n, cap in ((3 * P - 7, 3), (3 * P - 7, 2), (3 * P - 7, 1), (17 * P + 3, 16)):
        env = dict(dirs, DPGO_GRID_UPDATE=str(cap))
        for path in (VC32, VCPLAIN):
            rec, _ = both_orders(oracle, d, r, n, path, env, RTR_iterations=2, RTR_tCG_iterations=5)
            assert rec[8] > 0, rec


EXITS = {
    "residual": (dict(RTR_iterations=3, RTR_tCG_iterations=50), (TC.LCON, TC.SCON)),
    "boundary": (dict(RTR_iterations=3, RTR_tCG_iterations=50, RTR_initial_radius=1e-3), (TC.EXCR,)),
    "budget": (dict(RTR_iterations=3, RTR_tCG_iterations=2), (TC.MAXIT,)),
}
# (the residual test ends the runs of the V-cycle on smallGrid3D from the chordal start, tests/test_tcg_feed_gpu.py; block-
# Jacobi, whose instances have no pipelined form, is not held to an exit there)
EXIT_CASES = [(e, p) for e in sorted(EXITS) for p in (VC32, VC64, VCPLAIN, JACOBI) if (e, p) != ("residual", JACOBI)]


@pytest.mark.parametrize("dirs", [KEPT, SUMMED], ids=["kept", "summed"])
@pytest.mark.parametrize("exit_,path", EXIT_CASES)
def test_every_exit_of_tcg(oracle, exit_, path, dirs):
    """The runs end on the boundary step from a radius of 1e-3 (the kernel's mode 1 is the last launch of every run, with a
    tile in flight behind it) and on a budget of two products: (3, 5) and (3, 4) on 200 poses; on the residual test:
    smallGrid3D (125 poses, r = 5) from the chordal start."""
    prm, statuses = EXITS[exit_]
    if exit_ == "residual":
        from test_tcg_feed_gpu import SMALL, start_of
        blocks = [(3, SMALL.r, TC.build_problem(oracle, SMALL)["n"], (TC.build_problem(oracle, SMALL)["om"], start_of(oracle, SMALL)[0]))]
    else:
        blocks = [(3, 5, 200, None), (3, 4, 200, None)]
    for d, r, n, problem in blocks:  # (200 and 125 poses under one update workgroup: four and two tiles in it)
        rec, status = both_orders(oracle, d, r, n, path, dict(dirs, DPGO_GRID_UPDATE="1"), problem=problem, **prm)
        assert status in statuses and rec[8] >= rec[6] > 0, (exit_, path, status, rec)  # (every run has a product)


@pytest.mark.parametrize("dirs", [KEPT, SUMMED], ids=["kept", "summed"])
def test_negative_curvature(oracle, dirs):
    """sphere2500 at r = 5 from a random point, V-cycle (the trust-region table's window: negative curvature twice, both
    steps rejected -- the boundary step along a direction of negative curvature, then a new run from the same iterate)."""
    case = TC.by_name("sphere2500-multilevel-k0")
    p = TC.build_problem(oracle, case)
    X0, radius = TC.window_start(oracle, case)
    prm = dict(RTR_iterations=len(case.expect), RTR_tCG_iterations=case.tcg_iterations, RTR_initial_radius=radius,
               gradnorm_tol=1e-2, problem=(p["om"], X0))
    for path in (VC32, VCPLAIN):
        rec, status = both_orders(oracle, p["d"], case.r, p["n"], path, dict(dirs, DPGO_GRID_UPDATE="16"), **dict(prm))
        assert status == TC.NEGC and rec[6:8] == (2, 0), (path, status, rec)  # (two outer iterations, none accepted)
