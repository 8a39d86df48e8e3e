"""np.longdouble restatement of the six robust costs of the device re-weighting (kernels/agent.h: k_edge_robust,
k_edge_robust_finish), used by tests/test_robust_cost*.py, with a-priori bounds for the device's fp64 results.  The weight
functions are RobustCost::weight (reference src/DPGO_robust.cpp:54-98); the rho functions are this project's (the reference
defines weights only), normalised so that rho'(r) / r is the weight.  Nothing here calls the oracle's fp64 code.

    type      weight w(r)                      rho(r)
    L2        1                                r^2 / 2
    L1        1 / r                            r
    Huber(c)  r < c ? 1 : c / r                r < c ? r^2 / 2 : c r - c^2 / 2
    TLS(c)    r < c ? 1 : 0                    min(r^2, c^2) / 2
    GM        1 / (1 + r^2)^2                  r^2 / (2 (1 + r^2))
    GNC_TLS   r^2 <= lo ? 1 : r^2 >= up ? 0    r^2 / 2 | b r sqrt(mu (mu + 1)) - mu (b^2 + r^2) / 2 | b^2 / 2
              : sqrt(b^2 mu (mu + 1) / r^2) - mu       with lo = mu / (mu + 1) b^2, up = (mu + 1) / mu b^2

Bounds (EPS = 2^-52, one unit in the last place of a result in [1, 2): every operation of the kernel -- sqrt and the division
included -- is allowed a relative error of EPS; U = 2^-53 is used for plain additions in a sum.  k counts the operations a
relative error passes through, an error of the argument of a square counted twice; none is fitted to a measurement).

* weight from the device's own rsq, |w_dev - w| <= k EPS w:
    L1       sqrt, division                                                                       k = 2
    Huber    sqrt, division (the branch r >= c; the other one is exact)                            k = 2
    GM       r: 1, r r: 2 + 1 = 3, a = 1 + r r: <= 3 + 1 = 4 on a, a a: 8 + 1 = 9, 1 / (a a): 10    k = 10
    GNC_TLS  r r: 3; b b: 1, (b b) mu: 2, mu + 1: 1, their product: 4; divided by r r: 8; sqrt: 4 + 1 = 5 on
             s = w + mu; s - mu: one more on w.  |dw| <= 5 EPS (w + mu) + EPS w <= 6 EPS (w + mu)  k = 6 on w + mu
    L2, TLS  exact.
  Which branch an edge takes is decided in fp64 (r against c; r r against lo, up as the kernel forms them): an edge within 4
  ulp of a threshold may take either neighbouring branch (near_threshold); further away the saturated values 1.0 and 0.0 are
  exact.

* one cost term rho(r) from the device's rsq, |d rho| <= k EPS mag with mag the sum of the magnitudes of the terms:
    L2 3 (sqrt, r r: 3; the halving is exact)   L1 1   TLS 3   Huber 4 (c r: 2, c c: 1, difference: 1, on c r + c^2 / 2)
    GM 8 (r r: 3, 1 + r r: 4, quotient: 3 + 4 + 1)   GNC_TLS 7 (A = b r sqrt(mu (mu + 1)): mu + 1: 1, product: 2, sqrt: 2,
    b r: 2, A: 5; B = mu (b b + r r) / 2: sum <= 4, product 5; A - B: 6 on A + B; one spare)   a fixed edge w rsq / 2: 2.

* the device's rsq against the longdouble residual: reweighting_reference.rsq_bound.  rho is monotone in rsq, so the
  propagated bound of a term is max |rho(rsq +- bound) - rho(rsq)|, evaluated, not linearised (L1 is not Lipschitz at 0).

* the sum: a lane adds its ceil(m / (256 g)) terms in sequence, the wave's shifts add 7 levels, the four waves 3, the finish
  kernel ceil(g / 256) + 7 + 3 more: depth(m, g) additions at most on any term, |d sum| <= depth U sum |term| (1 + depth U).
"""
import collections

import numpy as np

import reweighting_reference as ref

LD = np.longdouble
EPS = 2.0 ** -52
U = 2.0 ** -53
TYPES = ("L2", "L1", "TLS", "Huber", "GM", "GNC_TLS")  # order of RobustCostParameters::Type = the C ABI's numbers
K_WEIGHT = {"L2": 0, "L1": 2, "TLS": 0, "Huber": 2, "GM": 10, "GNC_TLS": 6}
K_RHO = {"L2": 3, "L1": 1, "TLS": 3, "Huber": 4, "GM": 8, "GNC_TLS": 7}
K_FIXED = 2

Cost = collections.namedtuple("Cost", "type mu barc huber tls", defaults=(1e-4, 5.0, 3.0, 10.0))


def _ld(a):
    return np.asarray(a, dtype=LD)


def gnc_bounds(cost):
    """(lo, up) on r^2 in longdouble."""
    mu, b2 = LD(cost.mu), LD(cost.barc) * LD(cost.barc)
    return mu / (mu + 1) * b2, (mu + 1) / mu * b2


def weight(cost, r):
    r = _ld(r)
    one, zero = np.ones_like(r), np.zeros_like(r)
    t = cost.type
    with np.errstate(divide="ignore", invalid="ignore"):
        if t == "L2":
            return one
        if t == "L1":
            return 1 / r
        if t == "Huber":
            return np.where(r < LD(cost.huber), one, LD(cost.huber) / r)
        if t == "TLS":
            return np.where(r < LD(cost.tls), one, zero)
        if t == "GM":
            a = 1 + r * r
            return 1 / (a * a)
        if t == "GNC_TLS":
            lo, up = gnc_bounds(cost)
            mu, b2 = LD(cost.mu), LD(cost.barc) * LD(cost.barc)
            mid = np.sqrt(b2 * mu * (mu + 1) / (r * r)) - mu
            return np.where(r * r >= up, zero, np.where(r * r <= lo, one, mid))
    raise ValueError(t)


def rho_terms(cost, r):
    """(rho(r), mag): mag = sum of the magnitudes of the terms rho is formed from (the bound K_RHO EPS mag refers to it)."""
    r = _ld(r)
    t = cost.type
    sq = r * r
    if t == "L2":
        return sq / 2, sq / 2
    if t == "L1":
        return r, r
    if t == "Huber":
        c = LD(cost.huber)
        return np.where(r < c, sq / 2, c * r - c * c / 2), np.where(r < c, sq / 2, c * r + c * c / 2)
    if t == "TLS":
        v = np.minimum(sq, LD(cost.tls) * LD(cost.tls)) / 2
        return v, v
    if t == "GM":
        v = sq / (2 * (1 + sq))
        return v, v
    if t == "GNC_TLS":
        lo, up = gnc_bounds(cost)
        mu, b = LD(cost.mu), LD(cost.barc)
        A, B = b * r * np.sqrt(mu * (mu + 1)), mu * (b * b + sq) / 2
        return (np.where(sq >= up, b * b / 2, np.where(sq <= lo, sq / 2, A - B)),
                np.where(sq >= up, b * b / 2, np.where(sq <= lo, sq / 2, A + B)))
    raise ValueError(t)


def rho(cost, r):
    return rho_terms(cost, r)[0]


def kinks(cost):
    """The values of r at which the formula of the cost changes."""
    if cost.type == "Huber":
        return [LD(cost.huber)]
    if cost.type == "TLS":
        return [LD(cost.tls)]
    if cost.type == "GNC_TLS":
        return [np.sqrt(v) for v in gnc_bounds(cost)]
    return []


def weight_bound(cost, w):
    """k EPS w (GNC_TLS: on w + mu) for the weights `w` of the reference."""
    w = _ld(w)
    return K_WEIGHT[cost.type] * EPS * (w + (LD(cost.mu) if cost.type == "GNC_TLS" else 0))


def near_threshold(cost, rsq_dev, ulps=4):
    """Edges whose fp64 comparison value lies within `ulps` of a threshold as the kernel forms it."""
    rsq = np.asarray(rsq_dev, dtype=np.float64)
    r = np.sqrt(rsq)
    if cost.type == "Huber" or cost.type == "TLS":
        c = np.float64(cost.huber if cost.type == "Huber" else cost.tls)
        return np.abs(r - c) <= ulps * np.spacing(c)
    if cost.type == "GNC_TLS":
        lower, upper = ref.tls_thresholds(cost.mu, cost.barc)
        return (np.abs(r * r - upper) <= ulps * np.spacing(upper)) | (np.abs(r * r - lower) <= ulps * np.spacing(lower))
    return np.zeros(rsq.shape, dtype=bool)


def weights_from_rsq(cost, rsq_dev):
    """(w, bound, near) from the device's own rsq."""
    w = weight(cost, np.sqrt(_ld(rsq_dev)))
    return w, weight_bound(cost, w), near_threshold(cost, rsq_dev)


def depth(m, grid):
    per_lane = -(-max(int(m), 1) // (256 * int(grid)))
    return per_lane + 10 + -(-int(grid) // 256) + 10


def default_grid(m):
    return max(1, min(1024, -(-int(m) // 256)))


def cost_reference(cost, rsq, rsq_bound, weights, fixed, counted, grid=None):
    """(sum, bound) of the cost the device reports: rho(r_e) of the non-fixed counted edges plus w_e rsq_e / 2 of the fixed
    counted ones.  rsq: longdouble residuals with their bound against the device's (reweighting_reference.residuals,
    rsq_bound); weights: the stored weights (only the fixed edges' are used); counted: edges that contribute (role != 2)."""
    rsq, eb = _ld(rsq), _ld(rsq_bound)
    fixed, counted = np.asarray(fixed, dtype=bool), np.asarray(counted, dtype=bool)
    m = len(rsq)
    if m == 0:
        return LD(0), LD(0)
    r = np.sqrt(rsq)
    val, mag = rho_terms(cost, r)
    hi = rho(cost, np.sqrt(rsq + eb))
    lo = rho(cost, np.sqrt(np.maximum(rsq - eb, 0)))
    prop = np.maximum(np.abs(hi - val), np.abs(lo - val))
    term_err = K_RHO[cost.type] * EPS * (mag + prop) + prop
    wf = _ld(weights)
    fval = wf * rsq / 2
    ferr = K_FIXED * EPS * np.abs(fval) + np.abs(wf) * eb / 2 * (1 + K_FIXED * EPS)
    terms = np.where(fixed, fval, val)[counted]
    errs = np.where(fixed, ferr, term_err)[counted]
    dep = depth(m, default_grid(m) if grid is None else grid)
    total = np.sum(terms)
    bound = np.sum(errs) + dep * U * (np.sum(np.abs(terms)) + np.sum(errs)) * (1 + dep * U)
    return total, bound


def to_c(L, cost):
    """The C ABI's dpgo_robust_cost of a Cost."""
    return L.RobustCostC(TYPES.index(cost.type), float(cost.mu), float(cost.barc), float(cost.huber), float(cost.tls))
