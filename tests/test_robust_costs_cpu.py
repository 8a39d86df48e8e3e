"""CPU-side checks of the robust-cost re-weighting: the C ABI's declarations, exports and ctypes mirrors, the refusal
without a device, and the DistributedRobustPGO driver over two gloo ranks with a host stand-in for the per-agent work (the
orchestration under test is the product's)."""
import ctypes as C
import os
import re
import socket
import sys

import numpy as np
import pytest

from conftest import ROOT, to_product_measurements
from test_distributed_cpu import HostGncAgent, _gnc_case

ENTRIES = ("dpgo_robust_cost_default", "dpgo_problem_robust_reweight_device", "dpgo_problem_robust_reweight")


def test_header_exports_and_bindings_agree_for_the_new_entries():
    import dpgo_amd.lib as L
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpgo_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dpgo_[a-zA-Z0-9_]+)\s*\(", hdr))
    for name in ENTRIES:
        assert name in declared and hasattr(lib, name) and name in L.SIGNATURES, name
    assert len(L.SIGNATURES["dpgo_problem_robust_reweight_device"][0]) == 7
    assert len(L.SIGNATURES["dpgo_problem_robust_reweight"][0]) == 6
    for k, name in enumerate(("L2", "L1", "TLS", "HUBER", "GM", "GNC_TLS")):
        assert re.search(r"#define\s+DPGO_COST_%s\s+%d\b" % (name, k), hdr), name
    assert L.COST_TYPES == {"L2": 0, "L1": 1, "TLS": 2, "Huber": 3, "GM": 4, "GNC_TLS": 5}
    opts = L.describe_options()
    assert "DPGO_GRID_EDGES=0" in opts


def test_struct_mirrors_match_the_library():
    """Sizes and field order: dpgo_robust_cost_default writes L2, mu 1e-4, barc 5, Huber 3, TLS 10 (the reference's
    defaults, include/DPGO/DPGO_robust.h:49-57) into the fields the ctypes mirror names, and nothing past them."""
    import dpgo_amd.lib as L
    from dpgo_amd.robust import RobustCost, RobustCostParameters
    from dpgo_amd.solver import robust_cost_to_c
    assert C.sizeof(L.RobustCostC) == 40 and C.sizeof(L.ReweightStatsC) == 32
    assert [f for f, _ in L.RobustCostC._fields_] == ["type", "mu", "barc", "huber_threshold", "tls_threshold"]
    assert [f for f, _ in L.ReweightStatsC._fields_] == ["inliers", "outliers", "undecided", "skipped", "max_rsq", "cost"]
    assert L.ReweightStatsC.max_rsq.offset == 16 and L.ReweightStatsC.cost.offset == 24

    class Padded(C.Structure):
        _fields_ = [("c", L.RobustCostC), ("guard", C.c_uint64)]
    p = Padded(L.RobustCostC(9, -1.0, -1.0, -1.0, -1.0), 0xFEEDFACECAFEBEEF)
    L.load().dpgo_robust_cost_default(C.cast(C.byref(p), C.POINTER(L.RobustCostC)))
    assert (p.c.type, p.c.mu, p.c.barc, p.c.huber_threshold, p.c.tls_threshold) == (0, 1e-4, 5.0, 3.0, 10.0)
    assert p.guard == 0xFEEDFACECAFEBEEF
    L.load().dpgo_robust_cost_default(None)  # tolerated
    d = RobustCostParameters()
    assert (d.GNCInitMu, d.GNCBarc, d.HuberThreshold, d.TLSThreshold) == (p.c.mu, p.c.barc, p.c.huber_threshold, p.c.tls_threshold)
    cost = RobustCost(RobustCostParameters("GNC_TLS", GNCBarc=2.0, GNCInitMu=0.5, HuberThreshold=7.0, TLSThreshold=9.0))
    cost.update()
    c = robust_cost_to_c(cost)
    assert (c.type, c.mu, c.barc, c.huber_threshold, c.tls_threshold) == (5, 0.5 * 1.4, 2.0, 7.0, 9.0)


def test_entry_refuses_without_a_device():
    """No handle can exist without a device; the entry says DPGO_ERR_HIP then (with a device: the null handle is the
    invalid argument)."""
    import dpgo_amd
    import dpgo_amd.lib as L
    lib = L.load()
    c, st = L.RobustCostC(), L.ReweightStatsC()
    lib.dpgo_robust_cost_default(C.byref(c))
    X = np.zeros((5, 8))
    want = L.ERR_INVALID if dpgo_amd.device_count() > 0 else L.ERR_HIP
    assert lib.dpgo_problem_robust_reweight_device(None, L.ptr(X), None, C.byref(c), 1e-8, 1, C.byref(st)) == want
    assert lib.dpgo_problem_robust_reweight(None, L.ptr(X), C.byref(c), 1e-8, 1, C.byref(st)) == want
    if want == L.ERR_HIP:
        assert b"device" in lib.dpgo_last_error().lower()


def test_driver_rejects_an_unknown_cost_type_before_touching_the_device():
    from dpgo_amd.robust import DistributedRobustPGO, RobustCost, RobustCostParameters
    from dpgo_amd.solver import robust_cost_to_c

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the cluster was touched: %s" % name)

    with pytest.raises(ValueError):
        DistributedRobustPGO(Untouchable(), RobustCostParameters("Cauchy"))
    with pytest.raises(ValueError):
        robust_cost_to_c(RobustCost(RobustCostParameters("Cauchy")))


# ---------------------------------------------------------------------------------------------
# DistributedRobustPGO over two gloo ranks (per-agent work: host formulas)
# ---------------------------------------------------------------------------------------------
class HostRobustProblem:
    """CPU stand-in for the re-weighting methods of dpgo_amd.QuadraticProblem that DistributedRobustPGO calls."""

    def __init__(self, agent):
        self.a = agent
        self.reweightable_index = None

    def _all(self):
        a = self.a
        return a.O.Measurements.concat([a.odo, a.priv, a.shared])

    def setReweightableEdges(self, include_shared=False):
        assert include_shared
        self.reweightable_index = np.arange(self._all().m)
        return len(self.reweightable_index)

    def setEdgeWeights(self, w):
        a = self.a
        k1, k2 = a.odo.m, a.odo.m + a.priv.m
        a.odo.weight[:], a.priv.weight[:], a.shared.weight[:] = w[:k1], w[k1:k2], w[k2:]

    def getEdgeWeights(self):
        m = self._all()
        return m.weight.copy(), np.zeros(m.m)

    def robustReweightDevice(self, X, nbr, cost, w_tol=1e-8, update=True):
        import robust_cost_reference as rc
        from dpgo_amd.solver import ReweightStats
        a = self.a
        m = self._all()
        d = m.d
        Xn, slot = X.numpy(), {pid: k for k, pid in enumerate(a.plan.slots[a.id])}
        rsq = np.zeros(m.m)
        for e in range(m.m):
            mine1, mine2 = m.r1[e] == a.id, m.r2[e] == a.id
            xi = Xn[m.p1[e]] if mine1 else nbr[slot[(int(m.r1[e]), int(m.p1[e]))]].numpy()
            xj = Xn[m.p2[e]] if mine2 else nbr[slot[(int(m.r2[e]), int(m.p2[e]))]].numpy()
            Yi, Yj = xi[:d].T, xj[:d].T
            rsq[e] = m.kappa[e] * np.sum((Yi @ m.R[e] - Yj) ** 2) + m.tau[e] * np.sum((xj[d] - xi[d] - Yi @ m.t[e]) ** 2)
        fixed = m.fixed | ((m.r1 == m.r2) & (m.p1 + 1 == m.p2))  # (the agent path never re-weights odometry)
        w = m.weight.copy()
        skipped = np.zeros(m.m, dtype=bool)
        if update:
            with np.errstate(divide="ignore"):
                wn = np.array([cost.weight(float(np.sqrt(v))) for v in rsq])
            skipped = ~fixed & ~np.isfinite(wn)
            take = ~fixed & ~skipped
            w[take] = wn[take]
            self.setEdgeWeights(w)
        p = cost.mParams
        c = rc.Cost(p.costType, cost.mu, p.GNCBarc, p.HuberThreshold, p.TLSThreshold)
        mine = m.r1 == a.id  # a shared edge is counted by the owner of its source pose
        terms = np.where(fixed, w * rsq / 2, np.asarray(rc.rho(c, np.sqrt(rsq)), dtype=np.float64))
        counted = ~fixed & mine & ~skipped
        wc = w[counted]
        n_out = int((wc < w_tol).sum())
        n_in = int(((wc >= w_tol) & (wc > 1 - w_tol)).sum())
        return ReweightStats(n_in, n_out, len(wc) - n_in - n_out, int((skipped & mine).sum()), float(rsq.max()),
                             float(terms[mine].sum()))


class HostRobustAgent(HostGncAgent):
    def __init__(self, *args):
        super().__init__(*args)
        self.problem = HostRobustProblem(self)

    def loop_closure_weights(self):
        return np.concatenate([self.priv.weight, self.shared.weight])


def _robust_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    import dpgo_oracle as O
    from dpgo_amd.agent import ExchangePlan, PGOAgentParameters, RBCDCluster, build_pose_graphs
    from dpgo_amd.robust import DistributedRobustPGO, RobustCostParameters
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        allm, n, X0, _ = _gnc_case(O)
        ranges, graphs = build_pose_graphs(to_product_measurements(allm), n, world, 5)
        _, per = O.partition_contiguous(allm, n, world)
        plan = ExchangePlan(graphs)
        s, e = ranges[rank]
        agent = HostRobustAgent(O, plan, rank, per[rank], X0[s:e], 5, 3)
        cluster = RBCDCluster(plan, {rank: agent}, rank, world)
        drv = DistributedRobustPGO(cluster, RobustCostParameters("Huber"),
                                   PGOAgentParameters(robustOptNumWeightUpdates=5, robustOptInnerIters=4, maxNumIters=30))
        info = drv.run()
        hist = np.array([[h["mu"], h["inliers"], h["outliers"], h["undecided"], h["skipped"], h["max_rsq"], h["cost"]]
                         for h in info["history"]])
        np.savez(os.path.join(out_dir, "robust%d.npz" % rank), hist=hist, updates=info["updates"], inner=info["inner_iterations"],
                 iterations=info["iterations"], final=info["robust_cost"], w=agent.problem.getEdgeWeights()[0])
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_huber_histories_agree_and_the_cost_never_rises(oracle, tmp_path):
    """DistributedRobustPGO("Huber") on the 5 x 4 x 3 grid with 6 outliers over two processes: both ranks record the same
    history (global counts and cost by all-reduce, shared edges counted once, the same decisions everywhere), exactly
    robustOptNumWeightUpdates updates, and the global robust cost never rises from one update to the next: Huber's rho is
    concave in r^2, so the weighted cost majorises it, and every block solve decreases the weighted cost.  Slack 1e-9 of the
    first cost for the rounding of the solver's own decrease test."""
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_robust_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    z = [np.load(os.path.join(str(tmp_path), "robust%d.npz" % k)) for k in range(2)]
    assert np.array_equal(z[0]["hist"], z[1]["hist"]) and np.array_equal(z[0]["inner"], z[1]["inner"])
    assert int(z[0]["updates"]) == int(z[1]["updates"]) == 5 == len(z[0]["hist"])
    assert int(z[0]["iterations"]) == int(z[1]["iterations"]) <= 30
    cost = z[0]["hist"][:, 6]
    slack = 1e-9 * cost[0]
    assert np.all(np.diff(cost) <= slack), cost
    assert float(z[0]["final"]) <= cost[-1] + slack and float(z[0]["final"]) == float(z[1]["final"])
    allm, n, _, m_clean = _gnc_case(oracle)
    robot = lambda p: np.minimum(p // (n // 2), 1)  # noqa: E731  (two contiguous halves)
    free = int((~(allm.fixed | ((robot(allm.p1) == robot(allm.p2)) & (allm.p1 + 1 == allm.p2)))).sum())  # each counted once
    assert np.all(z[0]["hist"][:, 1:5].sum(axis=1) == free) and np.all(z[0]["hist"][:, 4] == 0)
    assert (z[0]["hist"][-1, 3] > 0) and min(z[k]["w"].min() for k in range(2)) < 0.5  # some edge was down-weighted
