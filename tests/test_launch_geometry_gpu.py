"""Launch geometry of the SpMM-family kernels against fp64 references: every (d, r) at 1, 2 and 4 lane groups per pose
(DPGO_SPLIT) on pose counts around the workgroup tile, forced launch caps (DPGO_GRID_*) on both tile-walk branches of
tile_iter (kernels/common.h), caller pointers at an 8-byte offset (include/dpgo_hip.h, "Alignment"), and what a solve entry
leaves behind when the solve is refused after it has borrowed the caller's iterate.

Every output leaves through a buffer with a guard region of at least one workgroup tile before and after it: the result
region is prefilled with NaN, the guards with a sentinel bit pattern; a kernel that skips a tile leaves NaN, one that
stores past pose n - 1 changes a guard.  Inputs that stay on the device sit between NaN guards, so that a read past the
last pose poisons the result.  Tolerances are the parity suite's: element-wise 1e-11, scalars 1e-12, Q*V 1e-13 against
scipy's CSR product.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import certificate_reference as ref
from conftest import DATA, device_tcg_mode, matrix_to_tiles, tiles_to_matrix, to_product_measurements
from test_parity_gpu import RTOL_ELEM, _random_graph, relerr

pytestmark = pytest.mark.gpu

DR = [(2, 2), (2, 3), (2, 4), (2, 5), (3, 3), (3, 4), (3, 5), (3, 6)]  # DPGO_FOR_DR (csrc/host.h)
SPLITS = (1, 2, 4)
SENTINEL = 0x7FF4DEADBEEF0BAD  # a signalling-NaN bit pattern no kernel writes
GEOMETRY_VARS = ("DPGO_SPLIT", "DPGO_SPMM_SYMMETRIC", "DPGO_GRID_UPDATE", "DPGO_GRID_HESS", "DPGO_GRID_HESS_SYM",
                 "DPGO_GRID_RETRACT", "DPGO_GRID_OUTER_SYM", "DPGO_GRID_SPMM_SYM", "DPGO_GRID_ML", "DPGO_COARSE_GRID",
                 "DPGO_DENSE_CHUNK", "DPGO_PERSIST", "DPGO_RHO_EXACT", "DPGO_TCG_DIRS")


def tile_poses(d, split):
    """Poses per workgroup tile of a <D, R, SPLIT> kernel (Geo::P, kernels/common.h)."""
    return 4 * (64 // ((d + 1) * split))


def pose_counts(d, split):
    P = tile_poses(d, split)
    return sorted({1, 2, P - 1, P, P + 1, 17 * P + 3})  # (17 P + 3: 18 tiles, uneven XCD eighths)


@contextlib.contextmanager
def library_options(env):
    """The library's switches set to `env` (every geometry switch not in it unset), read again by dpgo_options_reload;
    handles created inside see them.  Restored whatever happens."""
    import dpgo_amd
    lib = dpgo_amd.lib.load()
    names = set(GEOMETRY_VARS) | set(env)
    saved = {k: os.environ.get(k) for k in names}
    try:
        for k in names:
            os.environ.pop(k, None)
        os.environ.update(env)
        dpgo_amd.lib.check(lib.dpgo_options_reload())
        text = dpgo_amd.lib.describe_options()
        assert all(("%s=%s [set]" % kv) in text for kv in env.items()), (env, text)
        yield lib
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        lib.dpgo_options_reload()


class Handle:
    """A problem handle on the C ABI with Q set from an oracle BSR (any symmetric block pattern with diagonal blocks)."""

    def __init__(self, lib, Qb, r, d):
        import dpgo_amd.lib as L
        self.lib, self.L, self.r, self.d, self.n = lib, L, r, d, Qb.n
        self.T = (d + 1) * r
        self.h = L._P()
        L.check(lib.dpgo_problem_create(C.byref(self.h), r, d, Qb.n, 0))
        L.check(lib.dpgo_problem_set_Q_bsr(self.h, Qb.nnzb, L.ptr(Qb.rowptr), L.ptr(Qb.colidx), L.ptr(Qb.vals)))

    def close(self):
        if self.h:
            self.lib.dpgo_problem_destroy(self.h)
            self.h = None

    def describe(self):
        buf = C.create_string_buffer(32768)
        self.L.check(self.lib.dpgo_problem_describe(self.h, buf, len(buf)))
        return buf.value.decode()

    def out(self, guard):
        return Guarded(self.n * self.T, guard, device=False)

    # host-pointer entries: X, V as [n, d+1, r] tiles (the bytes of the r x (d+1)n column-major matrix)
    def f(self, X):
        v = C.c_double()
        self.L.check(self.lib.dpgo_problem_f(self.h, self.L.ptr(np.ascontiguousarray(X)), C.byref(v)))
        return v.value

    def rie_grad_norm(self, X):
        v = C.c_double()
        self.L.check(self.lib.dpgo_problem_rie_grad_norm(self.h, self.L.ptr(np.ascontiguousarray(X)), C.byref(v)))
        return v.value

    def vec(self, entry, guard, *args):
        o = self.out(guard)
        self.L.check(getattr(self.lib, entry)(self.h, *[self.L.ptr(np.ascontiguousarray(a)) for a in args], o.ptr()))
        return o.result((self.n, self.d + 1, self.r))

    def jacobi(self, X, V, guard):
        o = self.out(guard)
        self.L.check(self.lib.dpgo_problem_precondition(self.h, self.L.PRECOND_BLOCK_JACOBI, 0.1,
                                                        self.L.ptr(np.ascontiguousarray(X)),
                                                        self.L.ptr(np.ascontiguousarray(V)), o.ptr()))
        return o.result((self.n, self.d + 1, self.r))

    def certificate_apply(self, X, V, guard):
        return self.vec("dpgo_problem_certificate_apply", guard, X, V)

    def set_G(self, G):
        self.L.check(self.lib.dpgo_problem_set_G(self.h, self.L.ptr(None if G is None else np.ascontiguousarray(G))))

    # device-pointer entries
    def spmm_device(self, Vd, guard, add_G=False):
        o = Guarded(self.n * self.T, guard, device=True)
        self.L.check(self.lib.dpgo_spmm_device(self.h, self.L.ptr(Vd), o.ptr(), int(add_G)))
        return o.result((self.n, self.d + 1, self.r))

    def eval_device(self, Xd):
        f, g = C.c_double(), C.c_double()
        self.L.check(self.lib.dpgo_problem_eval_device(self.h, self.L.ptr(Xd), C.byref(f), C.byref(g)))
        return f.value, g.value

    def eval_terms_device(self, Xd):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self.L.check(self.lib.dpgo_problem_eval_terms_device(self.h, self.L.ptr(Xd), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value


class Guarded:
    """`size` doubles between two guards of `guard` doubles (host numpy or device torch): the body prefilled with NaN, the
    guards with SENTINEL.  result() checks both and returns the body."""

    def __init__(self, size, guard, device, body=None, guard_nan=False):
        self.size, self.guard = size, guard
        host = np.empty(size + 2 * guard, dtype=np.float64)
        bits = host.view(np.uint64)
        bits[:] = np.uint64(SENTINEL)
        host[guard:guard + size] = np.nan if body is None else np.asarray(body, dtype=np.float64).reshape(-1)
        if guard_nan:
            host[:guard] = np.nan
            host[guard + size:] = np.nan
        if device:
            import torch
            self.buf = torch.from_numpy(host).to("cuda")
            self.body = self.buf[guard:guard + size]
            torch.cuda.synchronize()  # (the library's launches run on the handle's own stream)
        else:
            self.buf = host
            self.body = host[guard:guard + size]

    def ptr(self):
        import dpgo_amd.lib as L
        return L.ptr(self.body)

    def result(self, shape):
        if not isinstance(self.buf, np.ndarray):
            import torch
            torch.cuda.synchronize()
            host = self.buf.cpu().numpy()
        else:
            host = self.buf
        bits = host.view(np.uint64)
        g = self.guard
        assert np.all(bits[:g] == np.uint64(SENTINEL)), "store in front of the output"
        assert np.all(bits[g + self.size:] == np.uint64(SENTINEL)), "store behind the output"
        body = host[g:g + self.size]
        assert not np.isnan(body).any(), "output entries not written: %d" % int(np.isnan(body).sum())
        return body.reshape(shape).copy()


def device_input(a, guard):
    """A device copy of `a` between NaN guards (a read past the last pose poisons the result)."""
    return Guarded(a.size, guard, device=True, body=a, guard_nan=True).body


def guard_of(d, r):
    g = tile_poses(d, 1) * (d + 1) * r + 2
    return g + (g & 1)  # (even: the body keeps the buffer's 16-byte alignment)


_GRAPHS = {}


def graph_Q(oracle, d, n):
    """(Q, T): the block matrix of a random pose graph (_random_graph: odometry chain, loop closures, one hub row longer
    than the gather core's preloaded index window from 64 poses on) and its ground truth; n = 1: the first diagonal block
    of the two-pose graph."""
    key = (d, n)
    if key not in _GRAPHS:
        if n == 1:
            Q2, T2 = graph_Q(oracle, d, 2)
            b = d + 1
            Qb = oracle.BSR(1, b, np.array([0, 1]), np.array([0]), Q2.vals[:1].copy())
            _GRAPHS[key] = (Qb, T2[:1].copy())
        else:
            hub = 40 if n >= 64 else max(0, n - 4) // 2
            n_lc = n // 2 if n >= 8 else 0  # (_random_graph needs room for loop closures j > i + 1)
            om, T, _ = _random_graph(oracle, d, n, n_lc, hub, seed=700 + 10 * n + d)
            _GRAPHS[key] = (oracle.construct_Q(n, d, om), T)
    return _GRAPHS[key]


def point(oracle, T, d, r, seed):
    n = T.shape[0]
    rng = np.random.default_rng(seed)
    X = oracle.polar_project(oracle.lift(T, r) + 0.1 * rng.standard_normal((n, d + 1, r)), d)
    V = rng.standard_normal((n, d + 1, r))
    G = 0.1 * rng.standard_normal((n, d + 1, r))
    return X, V, G


def check_against_references(oracle, h, Qb, X, V, G, guard):
    """Every evaluation of the handle against the oracle / scipy in fp64; returns the element-wise outputs."""
    import torch
    d, r, n = h.d, h.r, h.n
    N = n * (d + 1)
    Qs = ref.sparse_Q(Qb)
    op = oracle.QuadraticProblem(Qb, None, r, d, precond="jacobi")
    QV = (Qs @ V.reshape(N, r)).reshape(V.shape)
    out = {}
    Vd = device_input(V, guard)
    Xd = device_input(X, guard)
    out["QV"] = h.spmm_device(Vd, guard)
    assert relerr(out["QV"], QV) < 1e-13
    assert abs(h.f(X) - op.f(X)) <= 1e-12 * abs(op.f(X))
    out["EucGrad"] = h.vec("dpgo_problem_euc_grad", guard, X)
    assert relerr(out["EucGrad"], op.euc_grad(X)) < RTOL_ELEM
    out["EucHess"] = h.vec("dpgo_problem_euc_hess", guard, V)
    assert relerr(out["EucHess"], QV) < 1e-13
    out["RieGrad"] = h.vec("dpgo_problem_rie_grad", guard, X)
    assert relerr(out["RieGrad"], op.rie_grad(X)) < RTOL_ELEM
    gn = op.rie_grad_norm(X)
    assert abs(h.rie_grad_norm(X) - gn) <= 1e-12 * gn
    S = op.sym_ytg(X, op.euc_grad(X))
    Vt = oracle.tangent_project(X, V, d)
    out["RieHess"] = h.vec("dpgo_problem_rie_hess", guard, X, Vt)
    assert relerr(out["RieHess"], op.rie_hess(X, S, Vt)) < RTOL_ELEM
    out["Jacobi"] = h.jacobi(X, V, guard)
    assert relerr(out["Jacobi"], op.precondition(X, V)) < RTOL_ELEM
    f, g = h.eval_device(Xd)
    assert abs(f - op.f(X)) <= 1e-12 * abs(op.f(X)) and abs(g - gn) <= 1e-12 * gn
    xqx, xg, g2 = h.eval_terms_device(Xd)
    assert abs(xqx - 2 * op.f(X)) <= 1e-12 * abs(2 * op.f(X)) and xg == 0.0 and abs(g2 - gn * gn) <= 1e-12 * gn * gn
    Xm, Vm = tiles_to_matrix(X), tiles_to_matrix(V)
    out["CertApply"] = h.certificate_apply(X, V, guard)
    want = ref.certificate_apply(Qs, Xm, Vm, d)
    assert np.linalg.norm(tiles_to_matrix(out["CertApply"]) - want) <= 1e-12 * np.linalg.norm(want)
    # with a linear term G (dpgo_problem_set_G): f(X) = 0.5 <XQ, X> + <X, G>
    h.set_G(G)
    opG = oracle.QuadraticProblem(Qb, G, r, d, precond="jacobi")
    out["QV+G"] = h.spmm_device(Vd, guard, add_G=True)
    assert relerr(out["QV+G"], QV + G) < 1e-13
    assert abs(h.f(X) - opG.f(X)) <= 1e-12 * abs(opG.f(X))
    out["EucGradG"] = h.vec("dpgo_problem_euc_grad", guard, X)
    assert relerr(out["EucGradG"], opG.euc_grad(X)) < RTOL_ELEM
    out["RieGradG"] = h.vec("dpgo_problem_rie_grad", guard, X)
    assert relerr(out["RieGradG"], opG.rie_grad(X)) < RTOL_ELEM
    gnG = opG.rie_grad_norm(X)
    f, g = h.eval_device(Xd)
    assert abs(f - opG.f(X)) <= 1e-12 * abs(opG.f(X)) and abs(g - gnG) <= 1e-12 * gnG
    xqx, xg, g2 = h.eval_terms_device(Xd)
    want_xg = float(np.sum(X * G))
    assert abs(xqx - 2 * op.f(X)) <= 1e-12 * abs(2 * op.f(X)) and abs(xg - want_xg) <= 1e-12 * np.sum(np.abs(X * G))
    assert abs(g2 - gnG * gnG) <= 1e-12 * gnG * gnG
    h.set_G(None)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------- A. every (d, r) x split x pose count
# launch caps of the matrix: none (grid = tiles up to the resident count), small ones (the plain-stride walk takes several
# trips on every pose count above the cap) and 16 / 17 (the XCD-eighths walk with uneven eighths on 17 P + 3 poses)
MATRIX_CAPS = [{}, {"DPGO_GRID_UPDATE": "3", "DPGO_GRID_HESS": "2"}, {"DPGO_GRID_UPDATE": "17", "DPGO_GRID_HESS": "16"}]
@pytest.mark.parametrize("d,r", DR)
def test_every_split_and_ragged_size_matches_fp64_references(oracle, d, r):
    """DPGO_SPLIT = 1, 2, 4 (a fresh handle per split and cap set, MATRIX_CAPS) on n = 1, 2, P - 1, P, P + 1, 17 P + 3
    poses, P the split's workgroup tile: k_spmm, k_grad, k_hess, k_precond and k_cert_apply through every evaluation entry, with and without G,
    against the oracle and scipy; guarded outputs.  In 2-D, r = 3 and r = 5 give odd tile sizes (generic stores), the
    other pairs the span path."""
    guard = guard_of(d, r)
    for split, caps in [(s, c) for s in SPLITS for c in MATRIX_CAPS]:
        with library_options(dict(caps, DPGO_SPLIT=str(split))) as lib:
            for n in pose_counts(d, split):
                Qb, T = graph_Q(oracle, d, n)
                X, V, G = point(oracle, T, d, r, seed=n + 31 * r)
                h = Handle(lib, Qb, r, d)
                try:
                    assert "lane groups per pose %d;" % split in h.describe()
                    check_against_references(oracle, h, Qb, X, V, G, guard)
                except AssertionError as e:
                    raise AssertionError("d=%d r=%d split=%d n=%d caps=%s: %s" % (d, r, split, n, caps, e)) from e
                finally:
                    h.close()


# ---------------------------------------------------------------- B. forced launch caps
CAP_SETS = [{k: str(c) for k in ("DPGO_GRID_UPDATE", "DPGO_GRID_HESS", "DPGO_GRID_HESS_SYM", "DPGO_GRID_OUTER_SYM",
                                  "DPGO_GRID_SPMM_SYM", "DPGO_GRID_ML", "DPGO_GRID_RETRACT")} for c in (1, 7, 15, 16, 17, 100)]
MIXED_CAPS = {"DPGO_GRID_UPDATE": "13", "DPGO_GRID_HESS": "5", "DPGO_GRID_HESS_SYM": "23", "DPGO_GRID_OUTER_SYM": "9",
              "DPGO_GRID_SPMM_SYM": "31", "DPGO_GRID_ML": "19", "DPGO_GRID_RETRACT": "3"}
CAP_SETS.append(MIXED_CAPS)


def _workload(oracle, name):
    if name.startswith("grid:"):
        om, n, _ = oracle.synthetic_grid(*[int(v) for v in name[5:].split("x")], seed=0)
    else:
        om, n = oracle.read_g2o(os.path.join(DATA, name + ".g2o"))
    return om, n


@pytest.mark.parametrize("name,split,storage", [("smallGrid3D", 4, "plain"), ("grid:40x40x25", 1, "plain"),
                                                ("grid:40x40x25", 1, "symmetric")])
def test_forced_launch_caps_keep_elementwise_outputs_bitwise(oracle, name, split, storage):
    """At a fixed split and storage every pose's output is computed by the same lanes whatever workgroup runs it: Q V,
    EucHessianEta, RieGrad, RieHessianEta, block-Jacobi and V C(X) are BIT-identical under every cap set -- 1, 7, 15
    (plain stride), 16, 17, 100 (XCD eighths, uneven) and a mixed set whose kernels write and reduce their partial sums on
    different grids -- to the uncapped run; f and |rgrad| (summation order changes with the grid) match the oracle."""
    om, n = _workload(oracle, name)
    d, r = om.d, 5
    Qb = oracle.construct_Q(n, d, om)
    Ttrue = np.zeros((n, d + 1, d))
    Ttrue[:, :d, :] = np.eye(d)
    X, V, _ = point(oracle, Ttrue, d, r, seed=5)
    Vt = oracle.tangent_project(X, V, d)
    op = oracle.QuadraticProblem(Qb, None, r, d, precond="jacobi")
    fo, gno = op.f(X), op.rie_grad_norm(X)
    guard = guard_of(d, r)
    base_env = {"DPGO_SPLIT": str(split), "DPGO_SPMM_SYMMETRIC": "1" if storage == "symmetric" else "0",
                "DPGO_PERSIST": "0"}
    Vd = device_input(V, guard)
    base = None
    for caps in [{}] + CAP_SETS:
        with library_options(dict(base_env, **caps)) as lib:
            h = Handle(lib, Qb, r, d)
            try:
                text = h.describe()
                assert "lane groups per pose %d;" % split in text
                in_use = C.c_int(-1)
                h.L.check(lib.dpgo_problem_set_spmm_variant(h.h, 0, C.byref(in_use)))  # DPGO_SPMM_AUTO
                assert in_use.value == (2 if storage == "symmetric" else 1), (storage, in_use.value)
                out = {"QV": h.spmm_device(Vd, guard), "EucHess": h.vec("dpgo_problem_euc_hess", guard, V),
                       "RieGrad": h.vec("dpgo_problem_rie_grad", guard, X),
                       "RieHess": h.vec("dpgo_problem_rie_hess", guard, X, Vt), "Jacobi": h.jacobi(X, V, guard),
                       "CertApply": h.certificate_apply(X, V, guard)}
                assert abs(h.f(X) - fo) <= 1e-12 * abs(fo), caps
                assert abs(h.rie_grad_norm(X) - gno) <= 1e-12 * gno, caps
            finally:
                h.close()
        if base is None:
            base = out
            assert relerr(out["QV"], op.euc_hess(V)) < 1e-13
            assert relerr(out["RieGrad"], op.rie_grad(X)) < RTOL_ELEM
            assert relerr(out["Jacobi"], op.precondition(X, V)) < RTOL_ELEM
        else:
            for k, v in out.items():
                assert np.array_equal(v.view(np.uint64), base[k].view(np.uint64)), (caps, k)


def test_certificate_under_split_2_and_caps_matches_default(oracle):
    """dpgo_problem_certify on solved smallGrid3D at 2 lane groups per pose and under the mixed cap set (multi-launch
    solve): the default run's status, lambda_min to 1e-10."""
    import dpgo_amd
    om, n = oracle.read_g2o(os.path.join(DATA, "smallGrid3D.g2o"))
    d, r = om.d, 5
    params = dict(eta=1e-6, tol_rel=1e-9, max_iterations=2000, precond="jacobi", seed=3)

    def problem():
        pg = dpgo_amd.PoseGraph(0, r, d)
        pg.setMeasurements(to_product_measurements(om))
        prob = dpgo_amd.QuadraticProblem(pg)
        prob.setPersistent(False)
        return prob

    with library_options({}):
        prob = problem()
        X = tiles_to_matrix(oracle.lift(oracle.chordal_initialization(om, n), r))
        opt = dpgo_amd.QuadraticOptimizer(prob, dpgo_amd.ROptParameters(precond="jacobi", gradnorm_tol=1e-8,
                                                                         RTR_iterations=200))
        for _ in range(5):
            X = opt.optimize(X)
            if opt.getOptResult().gradNormOpt <= 1e-8:
                break
        want = prob.certify(X, **params)
        del opt, prob
    for env in ({"DPGO_SPLIT": "2"}, dict(MIXED_CAPS, DPGO_SPLIT="2")):
        with library_options(env):
            prob = problem()
            assert "lane groups per pose 2;" in prob.describe()
            got = prob.certify(X, **params)
            assert got.status == want.status, (env, got.status, want.status)
            assert abs(got.lambda_min - want.lambda_min) <= 1e-10, (env, got.lambda_min, want.lambda_min)
            del prob


HANDOFF_CAPS = {"DPGO_GRID_UPDATE": "7", "DPGO_GRID_HESS": "3", "DPGO_GRID_RETRACT": "5"}
_SPHERE = {}


def _sphere_oracle(oracle, precond):
    """sphere2500 at r = 5 and the oracle's solves of test_optimize_matches_oracle_at_matched_settings from the lifted
    chordal initialisation (the device's tCG arithmetic, and the reference's); computed once per preconditioner."""
    if "graph" not in _SPHERE:
        om, n = oracle.read_g2o(os.path.join(DATA, "sphere2500.g2o"))
        Q = oracle.construct_Q(n, om.d, om)
        _SPHERE["graph"] = (om, n, Q, oracle.lift(oracle.chordal_initialization(om, n), 5))
    om, n, Q, X0 = _SPHERE["graph"]
    if precond not in _SPHERE:
        op = oracle.QuadraticProblem(Q, None, 5, om.d, precond=precond)
        oopt = oracle.QuadraticOptimizer(op, oracle.ROptParameters(), hess_recurrence=device_tcg_mode(n, om.d, 5))
        Xo = oopt.optimize(X0)
        ref_opt = oracle.QuadraticOptimizer(oracle.QuadraticProblem(Q, None, 5, om.d, precond=precond), oracle.ROptParameters())
        Xr = ref_opt.optimize(X0)
        Xa = np.abs(X0).reshape(-1, 5)
        _SPHERE[precond] = (oopt.result, Xo, ref_opt.result, Xr, float((Xa * (abs(op.Qs) @ Xa)).sum()))
    return (om, n, X0) + _SPHERE[precond]


@pytest.mark.parametrize("precond", ["jacobi", "none"])
def test_multi_launch_solve_hands_partial_sums_across_different_grids(oracle, precond):
    """sphere2500 on the multi-launch solve (one-launch solve off) without the V-cycle, under caps that bind on every kernel
    family -- 40 workgroup tiles for the update family, 157 at four lane groups per pose; update 7, Hessian step / k_grad /
    k_hess 3, retraction 5 -- with the rho test from tCG's residual (k_retract writes region H) and from a fresh H eta
    (k_hess does), with and without kept directions: every writer / reader pair of the partial-sum regions E, A, B and H
    runs on two different grids.  Each solve is the oracle's, by the counts, status and tolerances of
    test_optimize_matches_oracle_at_matched_settings; so is a second solve on the same handle, which starts from regions
    the first one left written."""
    import dpgo_amd
    om, n, X0, ro, Xo, rr, Xr, scale = _sphere_oracle(oracle, precond)
    d, r = om.d, 5
    for rho_exact, dirs in [(a, b) for a in (0, 1) for b in (0, 1)]:
        # (the defaults -- DPGO_RHO_EXACT 0, DPGO_TCG_DIRS 1 -- by leaving the switch unset: library_options unsets both)
        env = dict(HANDOFF_CAPS, **({"DPGO_RHO_EXACT": "1"} if rho_exact else {}), **({} if dirs else {"DPGO_TCG_DIRS": "0"}))
        with library_options(env):
            text = dpgo_amd.lib.describe_options()
            assert "DPGO_RHO_EXACT=%d" % rho_exact in text and "DPGO_TCG_DIRS=%d" % dirs in text, text
            pg = dpgo_amd.PoseGraph(0, r, d)
            pg.setMeasurements(to_product_measurements(om))
            prob = dpgo_amd.QuadraticProblem(pg)
            prob.setPersistent(False)
            assert "lane groups per pose 4;" in prob.describe()
            gopt = dpgo_amd.QuadraticOptimizer(prob, dpgo_amd.ROptParameters(precond=precond))
            for solve in (1, 2):
                Xg = matrix_to_tiles(gopt.optimize(tiles_to_matrix(X0)), d)
                rg = gopt.getOptResult()
                try:
                    assert rg.success
                    assert abs(rg.fInit - ro.fInit) <= 1e-14 * scale
                    assert abs(rg.gradNormInit - ro.gradNormInit) <= 1e-10 * ro.gradNormInit
                    assert rg.rtr_iterations == ro.outer_iters
                    assert rg.tcg_iterations == ro.tcg_iters
                    assert rg.tCGStatus == oracle.TCG_NAMES[ro.tCGStatus]
                    assert abs(rg.fOpt - ro.fOpt) <= 1e-9 * abs(ro.fOpt) + 1e-14 * scale
                    assert relerr(Xg, Xo) < 1e-7
                    assert abs(prob.f(tiles_to_matrix(Xg)) - rg.fOpt) <= 1e-12 * abs(rg.fOpt) + 1e-14 * scale
                    assert rr.outer_iters == rg.rtr_iterations
                    assert abs(rg.fOpt - rr.fOpt) <= 1e-7 * abs(rr.fOpt) + 1e-14 * scale
                    assert relerr(Xg, Xr) < 1e-5
                except AssertionError as e:
                    raise AssertionError("%s solve %d under %s: %s" % (precond, solve, env, e)) from e
            del gopt, prob


# ---------------------------------------------------------------- C. caller pointers at an 8-byte offset
@pytest.mark.parametrize("name,storage", [("smallGrid3D", "auto"), ("grid:40x40x25", "symmetric")])
def test_spmm_device_at_an_odd_element_offset(oracle, name, storage):
    """dpgo_spmm_device on float64 views at element offset 1 (8-byte, not 16-byte aligned): on the symmetric storage the
    product takes the plain kernel (the symmetric one stores 16-byte pieces), so it is BITWISE the aligned plain product;
    pointers that are not 8-byte aligned are refused."""
    import torch
    import dpgo_amd.lib as L
    om, n = _workload(oracle, name)
    d, r = om.d, 5
    Qb = oracle.construct_Q(n, d, om)
    T = (d + 1) * r
    V = np.random.default_rng(3).standard_normal((n, d + 1, r))
    Qs = ref.sparse_Q(Qb)
    want = (Qs @ V.reshape(-1, r)).reshape(V.shape)
    env = {"DPGO_SPMM_SYMMETRIC": "1"} if storage == "symmetric" else {}
    with library_options(env) as lib:
        h = Handle(lib, Qb, r, d)
        try:
            if storage == "symmetric":
                in_use = C.c_int(-1)
                L.check(lib.dpgo_problem_set_spmm_variant(h.h, 0, C.byref(in_use)))
                assert in_use.value == 2
            big_v = torch.zeros(n * T + 2, dtype=torch.float64, device="cuda")
            big_o = torch.full((n * T + 2,), float("nan"), dtype=torch.float64, device="cuda")
            big_v[1:1 + n * T] = torch.from_numpy(V.reshape(-1))
            assert big_v[1:].data_ptr() % 16 == 8 and big_o[1:].data_ptr() % 16 == 8
            aligned_v = torch.from_numpy(V.reshape(-1)).to("cuda")
            aligned_o = torch.empty_like(aligned_v)
            torch.cuda.synchronize()
            L.check(lib.dpgo_spmm_device(h.h, L.ptr(aligned_v), L.ptr(aligned_o), 0))
            L.check(lib.dpgo_spmm_device(h.h, L.ptr(big_v[1:]), L.ptr(big_o[1:]), 0))
            torch.cuda.synchronize()
            odd = big_o[1:1 + n * T].cpu().numpy()
            assert np.isnan(big_o[0].item()) and np.isnan(big_o[-1].item())
            assert relerr(odd.reshape(V.shape), want) < 1e-13
            if storage == "symmetric":  # the plain product, bit for bit
                L.check(lib.dpgo_problem_set_spmm_variant(h.h, 1, C.byref(in_use)))  # DPGO_SPMM_PLAIN
                L.check(lib.dpgo_spmm_device(h.h, L.ptr(aligned_v), L.ptr(aligned_o), 0))
                torch.cuda.synchronize()
            assert np.array_equal(odd.view(np.uint64), aligned_o.cpu().numpy().view(np.uint64))
            bad = big_v.data_ptr() + 4  # (never dereferenced: refused on the host)
            assert lib.dpgo_spmm_device(h.h, bad, L.ptr(aligned_o), 0) == L.ERR_INVALID
            assert lib.dpgo_spmm_device(h.h, L.ptr(aligned_v), bad, 0) == L.ERR_INVALID
        finally:
            h.close()


def test_device_solves_at_an_odd_element_offset(oracle):
    """dpgo_optimize_device, _begin / _end and _many on an iterate at element offset 1 (d = 3, r = 5: even tile size, the
    16-byte span kernels of tCG and the V-cycle): the solve runs on the handle's own buffer, copied in and out, and gives
    the aligned call's result; the entries that read the caller's buffer in 8-byte elements (eval, certify) agree
    bitwise.  A pointer that is not 8-byte aligned is refused."""
    import torch
    import dpgo_amd
    import dpgo_amd.lib as L
    om, n = oracle.read_g2o(os.path.join(DATA, "smallGrid3D.g2o"))
    d, r = om.d, 5
    T = (d + 1) * r
    X0 = np.ascontiguousarray(oracle.lift(oracle.chordal_initialization(om, n), r))
    pg = dpgo_amd.PoseGraph(0, r, d)
    pg.setMeasurements(to_product_measurements(om))
    results = {}
    for precond in ("multilevel", "jacobi"):
        for persistent in (False, True):
            prob = dpgo_amd.QuadraticProblem(pg)
            prob.setPersistent(persistent)
            opt = dpgo_amd.QuadraticOptimizer(prob, dpgo_amd.ROptParameters(precond=precond))
            aligned = torch.from_numpy(X0.reshape(-1)).to("cuda")
            torch.cuda.synchronize()
            ra = opt.optimizeDevice(aligned)
            big = torch.full((n * T + 2,), float("nan"), dtype=torch.float64, device="cuda")
            odd = big[1:1 + n * T]
            assert odd.data_ptr() % 16 == 8
            for entry in ("device", "begin_end", "many"):
                odd.copy_(torch.from_numpy(X0.reshape(-1)))
                torch.cuda.synchronize()
                if entry == "device":
                    ro = opt.optimizeDevice(odd)
                elif entry == "begin_end":
                    opt.optimizeDeviceBegin(odd)
                    ro = opt.optimizeDeviceEnd()
                else:
                    ro = dpgo_amd.solver.optimize_device_many([opt], [odd])[0]
                torch.cuda.synchronize()
                assert np.isnan(big[0].item()) and np.isnan(big[-1].item()), entry
                xo, xa = odd.cpu().numpy(), aligned.cpu().numpy()
                assert (ro.tcg_iterations, ro.rtr_iterations) == (ra.tcg_iterations, ra.rtr_iterations), (precond, entry)
                assert abs(ro.fOpt - ra.fOpt) <= 1e-9 * abs(ra.fOpt), (precond, entry)
                assert relerr(xo, xa) < 1e-6, (precond, entry)
                results[(precond, persistent, entry)] = ro.fOpt
            # eval and certify read X in 8-byte elements: bitwise the aligned call
            copy = odd.clone()
            torch.cuda.synchronize()
            assert prob.evalDevice(odd) == prob.evalDevice(copy)
            assert prob.evalTermsDevice(odd) == prob.evalTermsDevice(copy)
            bad = big.data_ptr() + 4  # (never dereferenced: refused on the host)
            cp, cr = L.RoptParamsC(), L.RoptResultC()
            prob._lib.dpgo_ropt_params_default(C.byref(cp))
            assert prob._lib.dpgo_optimize_device(prob.handle, C.byref(cp), bad, C.byref(cr)) == L.ERR_INVALID
            assert prob._lib.dpgo_optimize_device_begin(prob.handle, C.byref(cp), bad, None) == L.ERR_INVALID
            del opt, prob


# ---------------------------------------------------------------- D. a solve refused after the iterate was borrowed
_TINY = {}


def _tiny(oracle):
    """tinyGrid3D at r = 5: (pose graph, n, d, r, lifted chordal initialisation as a flat vector), built once."""
    if not _TINY:
        import dpgo_amd
        om, n = oracle.read_g2o(os.path.join(DATA, "tinyGrid3D.g2o"))
        pg = dpgo_amd.PoseGraph(0, 5, om.d)
        pg.setMeasurements(to_product_measurements(om))
        X0 = np.ascontiguousarray(oracle.lift(oracle.chordal_initialization(om, n), 5)).reshape(-1)
        _TINY["graph"] = (pg, n, om.d, 5, X0)
    return _TINY["graph"]


def _optimizers(pg, persistent, count):
    import dpgo_amd
    opts = []
    for _ in range(count):
        prob = dpgo_amd.QuadraticProblem(pg)
        prob.setPersistent(persistent)
        opts.append(dpgo_amd.QuadraticOptimizer(prob, dpgo_amd.ROptParameters(precond="jacobi")))
    return opts


def _solve_through(entry, opts, xs):
    import dpgo_amd
    if entry == "device":
        return [opts[0].optimizeDevice(xs[0])]
    if entry == "begin_end":
        opts[0].optimizeDeviceBegin(xs[0])
        return [opts[0].optimizeDeviceEnd()]
    return dpgo_amd.solver.optimize_device_many(opts, xs)


def _fresh_solve(oracle, entry, persistent):
    """(tcg_iterations, rtr_iterations, fOpt, iterate) per handle of the ordinary solve through `entry` on fresh handles and
    aligned iterates; computed once per (entry, persistent), the handles released before it returns."""
    key = (entry, persistent)
    if key not in _TINY:
        import torch
        pg, n, d, r, X0 = _tiny(oracle)
        opts = _optimizers(pg, persistent, 2 if entry == "many" else 1)
        xs = [torch.from_numpy(X0).to("cuda") for _ in opts]
        torch.cuda.synchronize()
        res = _solve_through(entry, opts, xs)
        torch.cuda.synchronize()
        _TINY[key] = [(q.tcg_iterations, q.rtr_iterations, q.fOpt, x.cpu().numpy()) for q, x in zip(res, xs)]
    return _TINY[key]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("persistent", [False, True])
@pytest.mark.parametrize("entry", ["device", "begin_end", "many"])
def test_refused_solve_returns_the_borrowed_iterate(oracle, entry, persistent, offset):
    """A solve that the host refuses AFTER the entry has borrowed the caller's iterate (an unknown preconditioner:
    ERR_INVALID; the additive preconditioner under RGD: ERR_UNSUPPORTED -- both found while the solve is planned, before any
    of its launches) leaves the whole guarded buffer bitwise as it was, allocates nothing, leaves no solve in flight, and
    hands the handle its own x1 back: the ordinary solve that follows through the same entry on the same handle is the
    fresh handle's (iteration counts equal, fOpt to 1e-9 relative, iterate to 1e-6 -- the odd-offset test's tolerances for
    "same solve, other buffer").  tinyGrid3D, d = 3, r = 5; aligned iterates and iterates at element offset 1 (staged)."""
    import torch
    import dpgo_amd.lib as L
    from dpgo_amd.solver import _ptr_array
    pg, n, d, r, X0 = _tiny(oracle)
    want = _fresh_solve(oracle, entry, persistent)
    opts = _optimizers(pg, persistent, len(want))
    lib = opts[0].problem_._lib
    handles = [o.problem_.handle for o in opts]
    guard = guard_of(d, r) + offset  # (an odd guard puts the body at an odd element offset)
    bufs = [Guarded(X0.size, guard, device=True, body=X0, guard_nan=True) for _ in opts]
    xs = [b.body for b in bufs]
    assert all(x.data_ptr() % 16 == 8 * offset for x in xs)
    before = [b.buf.cpu().numpy().view(np.uint64).copy() for b in bufs]

    def live():
        a, b = C.c_longlong(), C.c_longlong()
        L.check(lib.dpgo_debug_live_allocations(C.byref(a), C.byref(b)))
        return a.value, b.value

    def call(cp):
        if entry == "device":
            return lib.dpgo_optimize_device(handles[0], C.byref(cp), L.ptr(xs[0]), C.byref(L.RoptResultC()))
        if entry == "begin_end":
            return lib.dpgo_optimize_device_begin(handles[0], C.byref(cp), L.ptr(xs[0]), None)
        res = (L.RoptResultC * len(opts))()
        return lib.dpgo_optimize_device_many(len(opts), _ptr_array([h.value for h in handles]), C.byref(cp),
                                             _ptr_array([L.ptr(x) for x in xs]), None, None, res)

    for changes, code in (({"precond": 99}, L.ERR_INVALID),
                          ({"method": L.METHOD_RGD, "precond": L.PRECOND_ADDITIVE}, L.ERR_UNSUPPORTED)):
        cp = L.RoptParamsC()
        lib.dpgo_ropt_params_default(C.byref(cp))
        for k, v in changes.items():
            setattr(cp, k, v)
        held = live()
        assert call(cp) == code, changes
        assert live() == held, changes
        if entry == "begin_end":  # no solve is in flight
            assert lib.dpgo_optimize_device_end(handles[0], C.byref(L.RoptResultC())) == L.ERR_STATE
        torch.cuda.synchronize()
        for b, was in zip(bufs, before):
            assert np.array_equal(b.buf.cpu().numpy().view(np.uint64), was), changes

    res = _solve_through(entry, opts, xs)
    torch.cuda.synchronize()
    for q, b, was, (tcg, rtr, f, x) in zip(res, bufs, before, want):
        bits = b.buf.cpu().numpy().view(np.uint64)
        assert np.array_equal(bits[:guard], was[:guard]) and np.array_equal(bits[guard + X0.size:], was[guard + X0.size:])
        assert (q.tcg_iterations, q.rtr_iterations) == (tcg, rtr)
        assert abs(q.fOpt - f) <= 1e-9 * abs(f)
        assert relerr(b.body.cpu().numpy(), x) < 1e-6
