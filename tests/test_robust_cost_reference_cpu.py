"""The longdouble restatement of the robust costs (tests/robust_cost_reference.py) against itself and against the package's
host mirror: rho'(r) / r is the weight, rho is continuous at every threshold, the weights are RobustCost.weight."""
import numpy as np
import pytest

import robust_cost_reference as rc

LD = np.longdouble
COSTS = [rc.Cost("L2"), rc.Cost("L1"), rc.Cost("TLS", tls=2.5), rc.Cost("TLS"), rc.Cost("Huber", huber=0.75), rc.Cost("Huber"),
         rc.Cost("GM"), rc.Cost("GNC_TLS", mu=0.3, barc=2.0), rc.Cost("GNC_TLS", mu=4.0, barc=0.5), rc.Cost("GNC_TLS")]
GRID = np.concatenate([np.linspace(0.01, 3.0, 300), np.linspace(3.0, 60.0, 300), [1e-3, 1e2, 6e2]])


def _away(cost, r, rel=1e-3):
    keep = np.ones(len(r), dtype=bool)
    for k in rc.kinks(cost):
        keep &= np.abs(r - float(k)) > rel * max(float(k), 1.0)
    return r[keep]


@pytest.mark.parametrize("cost", COSTS, ids=lambda c: "%s-%g-%g-%g-%g" % c)
def test_rho_prime_over_r_is_the_weight(cost):
    """Central differences in longdouble with h = 1e-6 r (truncation h^2 rho''' / 6, rounding 2^-63 rho / h: both below
    1e-10 of rho' on this grid), away from the kinks by 1e-3."""
    r = _away(cost, GRID).astype(LD)
    h = LD(1e-6) * r
    slope = (rc.rho(cost, r + h) - rc.rho(cost, r - h)) / (2 * h)
    w = rc.weight(cost, r)
    assert len(r) > 500
    assert np.all(np.abs(slope / r - w) <= 1e-9 * np.maximum(w, 1e-3 / (r * r))), cost


@pytest.mark.parametrize("cost", [c for c in COSTS if rc.kinks(c)], ids=lambda c: "%s-%g-%g-%g-%g" % c)
def test_rho_is_continuous_at_every_threshold(cost):
    """|rho(k (1 + 1e-15)) - rho(k (1 - 1e-15))| <= |rho'| 2e-15 k <= 2e-15 k^2 (1 + rounding): no jump."""
    for k in rc.kinks(cost):
        a, b = rc.rho(cost, k * (1 - LD(1e-15))), rc.rho(cost, k * (1 + LD(1e-15)))
        assert abs(a - b) <= LD(4e-15) * k * k, (cost, k, a, b)


@pytest.mark.parametrize("cost", COSTS, ids=lambda c: "%s-%g-%g-%g-%g" % c)
def test_weights_equal_the_host_mirror(cost):
    from dpgo_amd.robust import RobustCost, RobustCostParameters
    host = RobustCost(RobustCostParameters(cost.type, GNCBarc=cost.barc, GNCInitMu=cost.mu, HuberThreshold=cost.huber,
                                           TLSThreshold=cost.tls))
    assert host.mu == cost.mu
    r = _away(cost, GRID, rel=1e-9)
    want = rc.weight(cost, r.astype(LD))
    got = np.array([host.weight(float(x)) for x in r])
    scale = want + (cost.mu if cost.type == "GNC_TLS" else 0)
    assert np.all(np.abs(got - want) <= 1e-15 * scale), (cost, float(np.max(np.abs(got - want) / np.maximum(scale, 1e-300))))


def test_bounds_are_the_documented_operation_counts():
    assert rc.K_WEIGHT == {"L2": 0, "L1": 2, "TLS": 0, "Huber": 2, "GM": 10, "GNC_TLS": 6}
    assert rc.K_RHO == {"L2": 3, "L1": 1, "TLS": 3, "Huber": 4, "GM": 8, "GNC_TLS": 7}
    assert rc.depth(424, 2) == 1 + 10 + 1 + 10 and rc.depth(424, 1) == 2 + 21 and rc.depth(18240, 72) == 1 + 21
    assert rc.default_grid(424) == 2 and rc.default_grid(18240) == 72 and rc.default_grid(0) == 1
    # the propagated residual bound is evaluated, not linearised: L1 at a zero residual
    c, b = rc.cost_reference(rc.Cost("L1"), [0.0, 4.0], [1e-20, 0.0], [1.0, 1.0], [False, False], [True, True])
    assert c == 2 and 1e-10 <= b <= 1.1e-10
    # a fixed edge contributes w rsq / 2, an edge that is not counted nothing
    c, _ = rc.cost_reference(rc.Cost("TLS", tls=1.0), [4.0, 4.0, 4.0], [0, 0, 0], [0.5, 1.0, 1.0], [True, False, False],
                             [True, True, False])
    assert c == 1.0 + 0.5
