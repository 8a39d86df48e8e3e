"""What the library holds on the device and in pinned memory (dpgo_debug_live_allocations): every owner of a buffer
gives it back -- at the destroy, at the points where a handle replaces buffers in place, and on error paths.  The counter
is the library's own (csrc/host.h, DevBuf / PinBuf); hipMemGetInfo would also see everybody else's work on the card."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

from conftest import DATA, tiles_to_matrix

pytestmark = pytest.mark.gpu


def live():
    import dpgo_amd.lib as L
    buffers, nbytes = C.c_longlong(-1), C.c_longlong(-1)
    L.check(L.load().dpgo_debug_live_allocations(C.byref(buffers), C.byref(nbytes)))
    return buffers.value, nbytes.value


def lattice2d(nx, ny, seed):
    """SE(2) measurements on an nx x ny lattice in snake order (odometry chain + the lattice's other edges)."""
    import dpgo_amd
    rng = np.random.default_rng(seed)
    idx = np.arange(nx * ny).reshape(ny, nx)
    idx[1::2] = idx[1::2, ::-1].copy()
    pairs = set()
    for y in range(ny):
        for x in range(nx):
            if x + 1 < nx:
                pairs.add((min(idx[y, x], idx[y, x + 1]), max(idx[y, x], idx[y, x + 1])))
            if y + 1 < ny:
                pairs.add((min(idx[y, x], idx[y + 1, x]), max(idx[y, x], idx[y + 1, x])))
    pairs = np.array(sorted(pairs), dtype=np.int64)
    m = len(pairs)
    th = rng.uniform(-np.pi, np.pi, m)
    R = np.stack([np.stack([np.cos(th), -np.sin(th)], -1), np.stack([np.sin(th), np.cos(th)], -1)], -2)
    z = np.zeros(m, dtype=np.int64)
    meas = dpgo_amd.RelativeSEMeasurements(2, z, pairs[:, 0].copy(), z.copy(), pairs[:, 1].copy(), R,
                                           rng.standard_normal((m, 2)), rng.uniform(1.0, 50.0, m),
                                           rng.uniform(1.0, 50.0, m), np.ones(m), np.zeros(m, dtype=bool))
    return meas, nx * ny


def workload(name):
    import dpgo_amd
    if name == "smallGrid3D":
        meas, n = dpgo_amd.read_g2o_file(os.path.join(DATA, "smallGrid3D.g2o"))
        return meas, n, 3, 5
    meas, n = lattice2d(10, 10, seed=7)
    return meas, n, 2, 3


def start_point(n, d, r, seed):
    """Tiles [n, d+1, r] on the manifold: identity rotations lifted by [I_d; 0], random translations."""
    X = np.zeros((n, d + 1, r))
    X[:, :d, :d] = np.eye(d)
    X[:, d, :] = np.random.default_rng(seed).standard_normal((n, r))
    return X


def destroy(prob):
    import dpgo_amd.lib as L
    L.check(prob._lib.dpgo_problem_destroy(prob._h))
    prob._h = L._P()


def walk(meas, n, d, r):
    """One pass over every owner of device / pinned memory.  Returns the counts seen on the way.

    The symmetric storage and the fp32 operator copies exist for handles with one lane group per pose only
    (DPGO_SPLIT=1 at creation), the additive layout for handles with four (the default at these sizes): a handle's lane
    groups are fixed when it is created, so the additive step runs on a second handle of the same walk."""
    import torch
    import dpgo_amd
    import dpgo_amd.lib as L
    lib = L.load()
    seen = {}
    X0 = start_point(n, d, r, seed=1)
    saved = os.environ.get("DPGO_SPLIT")
    os.environ["DPGO_SPLIT"] = "1"
    L.check(lib.dpgo_options_reload())
    try:
        assert "DPGO_SPLIT=1 [set]" in L.describe_options()
        pg = dpgo_amd.PoseGraph(0, r, d)
        pg.setMeasurements(meas)
        prob = dpgo_amd.QuadraticProblem(pg)
        seen["created"] = live()
        prob.setPersistent(False)
        # symmetric storage (SymQ, the tile walk) and one product on it
        assert prob.setSpmmVariant("symmetric") == "symmetric"
        Xd = torch.tensor(X0, device="cuda", dtype=torch.float64)
        out = torch.zeros_like(Xd)
        prob.spmmDevice(Xd, out)
        torch.cuda.synchronize()
        seen["symmetric"] = live()
        assert seen["symmetric"][0] > seen["created"][0]
        # the hierarchy: levels, A P, the dense level; a multilevel solve (the fp32 copies where the block can run them)
        prob.setupMultilevel()
        opt = dpgo_amd.QuadraticOptimizer(prob, dpgo_amd.ROptParameters(precond="multilevel"))
        res = opt.optimizeDevice(Xd)
        assert res.precond_used == "multilevel"
        if (d + 1) * r % 2 == 0:  # (the tCG-step kernel of the symmetric storage needs an even tile)
            assert prob.multilevelOperatorBits()["active"]
        seen["multilevel"] = live()
        assert seen["multilevel"][0] > seen["symmetric"][0]
        # re-weightable edges: registered, used once, registered again (the first set is released in place)
        assert prob.setReweightableEdges() > 0
        seen["edges"] = live()
        assert seen["edges"][0] > seen["multilevel"][0]
        prob.gncReweightDevice(Xd, None, mu=1.0, barc=10.0)
        prob.setReweightableEdges()
        assert live() == seen["edges"]
        # certificate (its own buffers live for the call only)
        before = live()
        prob.certify(tiles_to_matrix(Xd.cpu().numpy()), witness=False, precond="multilevel", max_iterations=3)
        assert live() == before
        # rotating probes, two sets each: the handle owns neither more nor less afterwards
        ms, sb = C.c_double(0.0), C.c_double(0.0)
        before = live()
        L.check(lib.dpgo_bench_hess_rotating(prob.handle, 2, 2, 1, C.byref(ms)))
        assert live() == before
        L.check(lib.dpgo_bench_spmm_rotating(prob.handle, 2, 2, 1, C.byref(ms), C.byref(sb)))
        assert live() == before
        prob.spmmDevice(Xd, out)  # (the handle's own operands are back in place: the product still runs on them)
        torch.cuda.synchronize()
        # exchange plan: created, run, destroyed
        T = (d + 1) * r
        src = torch.arange(n * T, device="cuda", dtype=torch.float64).reshape(n, T)
        idx = torch.tensor([3, 0, n - 1], device="cuda", dtype=torch.int32)
        dst = torch.zeros((3, T), device="cuda", dtype=torch.float64)
        plan = L._P()
        L.check(lib.dpgo_exchange_plan_create(C.byref(plan), r, d, 1, (C.c_void_p * 1)(L.ptr(src)),
                                              (C.c_void_p * 1)(L.ptr(idx)), (C.c_int * 1)(3),
                                              (C.c_void_p * 1)(L.ptr(dst)), 0))
        assert live()[0] == before[0] + 4
        L.check(lib.dpgo_exchange_plan_run(plan, None))
        torch.cuda.synchronize()
        assert torch.equal(dst, src[idx.long()])
        L.check(lib.dpgo_exchange_plan_destroy(plan))
        assert live() == before
        # a Q with another block pattern (the odometry chain alone): hierarchy, symmetric copy and edges go in place
        chain = dpgo_amd.PoseGraph(0, r, d)
        chain.setMeasurements(meas.select(np.nonzero(meas.p1 + 1 == meas.p2)[0]))
        rp, ci, v = chain.quadraticMatrix()
        assert len(ci) == 3 * n - 2
        L.check(lib.dpgo_problem_set_Q_bsr(prob.handle, len(ci), L.ptr(rp), L.ptr(ci), L.ptr(v)))
        seen["new_pattern"] = live()
        assert seen["new_pattern"][0] == seen["created"][0] and seen["new_pattern"][1] < seen["created"][1]
        destroy(prob)
        seen["destroyed_first"] = live()
    finally:
        if saved is None:
            os.environ.pop("DPGO_SPLIT", None)
        else:
            os.environ["DPGO_SPLIT"] = saved
        L.check(lib.dpgo_options_reload())
    # the additive layout: the default hierarchy is dropped and rebuilt with one aggregate per workgroup tile
    pg = dpgo_amd.PoseGraph(0, r, d)
    pg.setMeasurements(meas)
    prob = dpgo_amd.QuadraticProblem(pg)
    prob.setupMultilevel()
    Xd = torch.tensor(X0, device="cuda", dtype=torch.float64)
    res = dpgo_amd.QuadraticOptimizer(prob, dpgo_amd.ROptParameters(precond="multilevel")).optimizeDevice(Xd)
    assert res.precond_used == "multilevel"
    seen["second_multilevel"] = live()
    Xd.copy_(torch.tensor(X0))
    res = dpgo_amd.QuadraticOptimizer(prob, dpgo_amd.ROptParameters(precond="additive")).optimizeDevice(Xd)
    assert res.precond_used == "additive" and "additive layout" in prob.describe()
    seen["additive"] = live()
    assert seen["additive"][0] > seen["destroyed_first"][0]
    destroy(prob)
    seen["destroyed"] = live()
    return seen


@pytest.mark.parametrize("name", ["smallGrid3D", "lattice2d"])
def test_every_owner_returns_its_memory(name):
    """A handle walked through every owner of device and pinned memory -- symmetric storage, hierarchy with its dense
    level and fp32 copies, the additive layout that replaces it, re-weightable edges registered twice, the certificate,
    both rotating probes, an exchange plan, a Q of another pattern -- on smallGrid3D (r = 5) and on a 100-pose SE(2)
    lattice at r = 3.  After the destroy the library holds exactly the buffers and bytes it held before, three walks in a
    row; while a handle lives it holds more; a rotating probe leaves the handle with exactly what it had."""
    meas, n, d, r = workload(name)
    gc.collect()  # (handles of earlier tests that are garbage go now, not in the middle of a walk)
    base = live()
    for rep in range(3):
        seen = walk(meas, n, d, r)
        assert seen["created"][0] > base[0] and seen["created"][1] > base[1], (rep, seen)
        assert seen["additive"][0] > base[0], (rep, seen)
        assert seen["destroyed_first"] == base, (rep, seen, base)
        assert seen["destroyed"] == base, (rep, seen, base)
        assert live() == base


def test_failed_calls_leave_no_allocation():
    """Error paths that return without a fault: the count is what it was before the call."""
    import torch
    import dpgo_amd.lib as L
    lib = L.load()
    wg, steps = 4, 1
    a = torch.zeros((wg, 256, 2), dtype=torch.float64, device="cuda")
    pw = torch.zeros((wg, 4, 7), dtype=torch.float64, device="cuda")
    sums = torch.zeros((wg, steps, 2), dtype=torch.float64, device="cuda")
    pout = torch.zeros((wg, steps, wg, 7), dtype=torch.float64, device="cuda")
    rows = torch.zeros((wg, 4, 7), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gc.collect()
    before = live()
    rc = lib.dpgo_debug_reduction_primitives(wg, 7, steps, L.ptr(a), L.ptr(pw), L.ptr(sums), L.ptr(pout), L.ptr(rows))
    assert rc == L.ERR_UNSUPPORTED
    assert live() == before
    idx = torch.zeros(3, dtype=torch.int32, device="cuda")
    dst = torch.zeros((3, 20), dtype=torch.float64, device="cuda")
    plan = L._P()
    rc = lib.dpgo_exchange_plan_create(C.byref(plan), 5, 3, 1, (C.c_void_p * 1)(None), (C.c_void_p * 1)(L.ptr(idx)),
                                       (C.c_int * 1)(3), (C.c_void_p * 1)(L.ptr(dst)), 0)
    assert rc == L.ERR_INVALID and not plan.value
    assert live() == before
