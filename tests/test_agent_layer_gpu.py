"""The device kernels that run between two local solves of a multi-robot sweep (csrc/agents.hip, csrc/kernels/agent.h)
against the references of tests/agent_layer_reference.py, at every (d, r) and at their launch edges:

A. the pose movers -- dpgo_gather_tiles_device, dpgo_permute_tiles_device, dpgo_exchange_plan_* -- bit for bit;
B. the coupling product G = G0 + Xnbr C (k_spmm on the rectangular operator of dpgo_problem_set_G_coupling) at 1, 2 and 4
   lane groups per pose against its longdouble value and forward error bound, and the same G on the entries that refresh it
   themselves (dpgo_problem_eval_terms_device_many, dpgo_optimize_device_many);
C. the relative change of the iterate (k_max_translation_distance);
D. the ordering words (dpgo_flags_write_device, dpgo_flags_wait_device_checked), one process, one stream, every wait for
   a value that an earlier launch on the same stream has already written, with a time limit and an error word;
E. the block-Jacobi factors (k_build_dinv) against longdouble inverses.

Outputs sit in guarded buffers prefilled with NaN (Guarded, tests/test_launch_geometry_gpu.py), device inputs between NaN
guards; index tables are padded with the index of the first guard tile, so that an index read past either end of the
table delivers NaN.  Grid-stride branches reached: k_gather_tiles / k_scatter_tiles (more than 1 024 x 256 elements),
k_gather_tiles_batched (more than 65 536 tiles, T = 6), k_spmm (more than 1 024 tiles, every split), and
k_max_translation_distance (more than 262 144 poses).  The eight (d, r) give T = 6, 9, 12, 15, 12, 16, 20, 24: all seven
instances of k_gather_tiles_batched.

Measured on an MI355X (the tests print these figures and put them into their failure messages):
  B, largest error / bound at split 1, 2, 4     C, largest relative error / ((r + 2) 2^-53)
    (2, 2)  0.483  0.475  0.465                   0.332
    (2, 3)  0.538  0.550  0.532                   0.195
    (2, 4)  0.575  0.575  0.575                   0.141
    (2, 5)  0.554  0.511  0.584                   0.166
    (3, 3)  0.497  0.491  0.491                   0.263
    (3, 4)  0.457  0.462  0.457                   0.195
    (3, 5)  0.575  0.475  0.465                   0.136
    (3, 6)  0.550  0.473  0.495                   0.137
  E, max |Dinv - exact| / max |exact| per class of kappa_2(Q_ii + shift I): device, np.linalg.inv (shift 0.1; 1e-3)
    d = 2  1e0 .. 7e1: 5.0e-16, 4.2e-16; 9.2e-16, 4.8e-16   3e3 .. 2e4: 6.3e-14, 1.4e-13; 7.9e-14, 1.1e-13
           2e7 .. 1e8: 1.9e-16, 1.5e-16; 1.9e-16, 1.9e-16
    d = 3  1e0 .. 5e1: 3.1e-16, 2.6e-16; 2.0e-16, 2.0e-16   3e3 .. 3e4: 3.4e-13, 3.8e-13; 2.5e-13, 4.3e-13
           2e7 .. 3e7: 2.5e-14, 1.1e-13; 5.2e-14, 5.6e-14
(the blocks' condition numbers are those of kappa, tau in {1, 1e4, 1e8}: the smallest eigenvalue of every block is of
order 1, so neither shift moves them.)
"""
import ctypes as C

import numpy as np
import pytest

import agent_layer_reference as A
from test_agent_layer_reference_cpu import jacobi_bsr
from test_launch_geometry_gpu import DR, SPLITS, Guarded, Handle, device_input, graph_Q, guard_of, library_options, point, \
    tile_poses

pytestmark = pytest.mark.gpu

NAN = float("nan")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def index_table(idx, n):
    """A device copy of idx with 64 entries of value n (the first tile of the source's NaN guard) in front and behind."""
    import torch
    pad = np.full(64, n, dtype=np.int32)
    buf = torch.from_numpy(np.concatenate([pad, np.asarray(idx, dtype=np.int32), pad])).to("cuda")
    return buf[64:64 + len(idx)]


def untouched(buf):
    """A Guarded whose body nobody may have written: NaN still, guards intact."""
    import torch
    torch.cuda.synchronize()
    host = buf.buf.cpu().numpy()
    g = buf.guard
    want = Guarded(buf.size, g, device=False).buf
    return np.array_equal(host.view(np.uint64), want.view(np.uint64))


# ================================================================ A. pose movers
@pytest.mark.parametrize("d,r", DR)
def test_gather_tiles_is_plain_indexing(d, r):
    """dpgo_gather_tiles_device: 1, 63, 64, 65, 257 tiles and a count past 1 024 x 256 elements (second grid-stride trip),
    idx with duplicates, 0 and n - 1, a source larger than what is gathered; both buffers at element offset 0 and 1;
    count = 0 writes nothing."""
    import dpgo_amd.lib as L
    lib = L.load()
    T = (d + 1) * r
    rng = np.random.default_rng(10 * d + r)
    for count, offset in [(c, 0) for c in A.GATHER_COUNTS + (A.gather_big_count(T),)] + [(65, 1), (257, 1)]:
        guard = guard_of(d, r) + offset
        n = count + 37
        src = A.tiles(rng, n, T)
        idx = A.gather_indices(n, count, seed=count)
        src_d, idx_d = device_input(src, guard), index_table(idx, n)
        out = Guarded(count * T, guard, device=True)
        assert src_d.data_ptr() % 16 == 8 * offset and out.body.data_ptr() % 16 == 8 * offset
        L.check(lib.dpgo_gather_tiles_device(r, d, L.ptr(src_d), L.ptr(idx_d), count, out.ptr(), None))
        assert same_bits(out.result((count, T)), A.gather(src, idx)), (count, offset)
    out = Guarded(T, guard_of(d, r), device=True)
    assert lib.dpgo_gather_tiles_device(r, d, L.ptr(src_d), L.ptr(idx_d), 0, out.ptr(), None) == L.OK
    assert lib.dpgo_gather_tiles_device(r, d, None, None, 0, None, None) == L.OK
    assert untouched(out)


@pytest.mark.parametrize("d,r", DR)
def test_permute_tiles_forward_and_back(d, r):
    """dpgo_permute_tiles_device with a random permutation at n = 1, P - 1, P, P + 1 and one n past the grid cap: forward
    is scatter, forward = 0 is gather, the inverse applied to the forward result is the input; offsets 0 and 1; in == out
    is refused and the buffer untouched."""
    import dpgo_amd.lib as L
    lib = L.load()
    T = (d + 1) * r
    P = tile_poses(d, 1)
    rng = np.random.default_rng(20 * d + r)
    for n, offset in [(k, 0) for k in (1, P - 1, P, P + 1, A.gather_big_count(T))] + [(P + 1, 1)]:
        guard = guard_of(d, r) + offset
        src = A.tiles(rng, n, T)
        perm = rng.permutation(n).astype(np.int32)
        src_d, perm_d = device_input(src, guard), index_table(perm, n)
        fwd, back, inv = (Guarded(n * T, guard, device=True) for _ in range(3))
        assert src_d.data_ptr() % 16 == 8 * offset and fwd.body.data_ptr() % 16 == 8 * offset
        L.check(lib.dpgo_permute_tiles_device(r, d, n, L.ptr(perm_d), L.ptr(src_d), fwd.ptr(), 1, None))
        assert same_bits(fwd.result((n, T)), A.scatter(src, perm)), (n, offset)
        L.check(lib.dpgo_permute_tiles_device(r, d, n, L.ptr(perm_d), fwd.ptr(), back.ptr(), 0, None))
        assert same_bits(back.result((n, T)), src), (n, offset)
        L.check(lib.dpgo_permute_tiles_device(r, d, n, L.ptr(perm_d), L.ptr(src_d), inv.ptr(), 0, None))
        assert same_bits(inv.result((n, T)), A.gather(src, perm)), (n, offset)
    same = Guarded(n * T, guard, device=True)
    for forward in (0, 1):
        assert lib.dpgo_permute_tiles_device(r, d, n, L.ptr(perm_d), same.ptr(), same.ptr(), forward, None) == L.ERR_INVALID
    assert untouched(same)
    assert lib.dpgo_permute_tiles_device(r, d, 0, None, None, None, 1, None) == L.OK


def _run_exchange(lib, d, r, name, offset):
    """One table through dpgo_exchange_plan_*: the destinations are slices of ONE guarded buffer, laid out in a shuffled
    message order; every other empty message passes null pointers.  Runs the plan, changes the sources, runs it again."""
    import torch
    import dpgo_amd.lib as L
    T = (d + 1) * r
    guard = guard_of(d, r) + offset
    rng = np.random.default_rng(len(name) + 100 * T)
    sizes, msgs = A.exchange_table(name)
    srcs = [A.tiles(rng, n, T) for n in sizes]
    srcs_d = [device_input(s, guard) for s in srcs]
    counts = [len(idx) for _, idx in msgs]
    total = sum(counts)
    order = rng.permutation(len(msgs))
    at = {}
    pos = 0
    for m in order:
        at[m] = pos
        pos += counts[m] * T
    out = Guarded(max(total, 1) * T, guard, device=True)
    idx_d = [index_table(idx, sizes[s]) for s, idx in msgs]
    empties = 0
    sp, ip, dp = [], [], []
    for m, (s, idx) in enumerate(msgs):
        null = False
        if counts[m] == 0:
            null = empties % 2 == 0
            empties += 1
        sp.append(None if null else L.ptr(srcs_d[s]))
        ip.append(None if null else L.ptr(idx_d[m]))
        dp.append(None if null else out.body.data_ptr() + 8 * at[m])
    nm = len(msgs)
    plan = L._P()
    L.check(lib.dpgo_exchange_plan_create(C.byref(plan), r, d, nm, (C.c_void_p * nm)(*sp), (C.c_void_p * nm)(*ip),
                                          (C.c_int * nm)(*counts), (C.c_void_p * nm)(*dp), 0))
    try:
        for sign in (1.0, -1.0):  # the second run: the same plan after every source changed (negated: exact)
            L.check(lib.dpgo_exchange_plan_run(plan, None))
            if total == 0:
                assert untouched(out), name
                continue
            got = out.result((total * T,))
            want = A.exchange([(sign * srcs[s], idx) for s, idx in msgs])
            for m in range(nm):
                assert same_bits(got[at[m]:at[m] + counts[m] * T].reshape(counts[m], T), want[m]), (name, offset, m, sign)
            for s_d in srcs_d:
                s_d.neg_()
            out.body.fill_(NAN)
            torch.cuda.synchronize()
    finally:
        L.check(lib.dpgo_exchange_plan_destroy(plan))


@pytest.mark.parametrize("d,r", DR)
def test_exchange_plan_delivers_every_message(d, r):
    """One launch of k_gather_tiles_batched<T> per table: 1, 2, 7 and 40 messages; empty messages first, in the middle (two
    in a row) and last, with and without pointers; messages of one tile; two messages that read overlapping poses; a plan
    whose total is zero; at T = 6 a table of more than 65 536 tiles (second grid-stride trip, a message boundary inside
    it); destinations at element offset 0 and 1.  Every slice is src[idx] bit for bit, before and after the sources
    change; nothing else is written."""
    import dpgo_amd.lib as L
    lib = L.load()
    for name in A.EXCHANGE_TABLES + ("all_empty",) + (("big",) if (d + 1) * r == 6 else ()):
        _run_exchange(lib, d, r, name, 0)
    _run_exchange(lib, d, r, "seven_empties", 1)


# ================================================================ B. coupling product
def _diag_Q(oracle, n, d):
    b = d + 1
    return oracle.BSR(n, b, np.arange(n + 1), np.arange(n), np.tile(np.eye(b), (n, 1, 1)))


class Coupled(Handle):
    """A handle with a coupling operator; G is read back exactly as Q 0 + G (dpgo_spmm_device, add_G = 1)."""

    def __init__(self, lib, Qb, r, d, guard):
        super().__init__(lib, Qb, r, d)
        self.guard = guard
        self.zero = device_input(np.zeros(self.n * self.T), guard)

    def set_coupling(self, ncols, rowptr, colidx, vals, G0):
        nnzb = len(colidx)
        self.L.check(self.lib.dpgo_problem_set_G_coupling(
            self.h, ncols, nnzb, self.L.ptr(rowptr), self.L.ptr(colidx) if nnzb else None,
            self.L.ptr(np.ascontiguousarray(vals)) if nnzb else None,
            None if G0 is None else self.L.ptr(np.ascontiguousarray(G0))))

    def update(self, nbr_d):
        self.L.check(self.lib.dpgo_problem_update_G_from_neighbors_device(self.h, self.L.ptr(nbr_d)))

    def G(self):
        return self.spmm_device(self.zero, self.guard, add_G=True)


def _coupling_case(n, ncols, d, r, seed):
    """(rowptr, colidx, vals, G0, [Xnbr first, Xnbr second], info) of one pattern."""
    rng = np.random.default_rng(seed)
    rowptr, colidx, info = A.coupling_pattern(n, ncols, d, seed)
    vals = rng.standard_normal((len(colidx), d + 1, d + 1))
    G0 = rng.standard_normal((n, d + 1, r))
    X = [rng.standard_normal((ncols, d + 1, r)) for _ in range(2)]
    return rowptr, colidx, vals, G0, X, info


def _check_G(dev, ref, G0, rowptr, b, what):
    """Rows without a block: G0 bit for bit (+0.0 without G0); every other element within (k + 2) 2^-53 mag.  Returns the
    largest error / bound."""
    G, mag = ref
    k = A.row_terms(rowptr, b)
    empty = k == 0
    want0 = np.zeros_like(dev[empty]) if G0 is None else G0[empty]
    assert same_bits(dev[empty], want0), "%s: a row without a block is not G0" % what
    if empty.all():
        return 0.0
    err = np.abs(np.array(dev[~empty], dtype=A.LD) - G[~empty])
    bound = ((k[~empty] + 2) * A.U)[:, None, None] * mag[~empty]
    ratio = float((err / bound).max())
    assert ratio <= 1.0, "%s: error / bound = %.3f" % (what, ratio)
    return ratio


_COUPLING_REFS = {}


def _coupling_ref(key, G0, rowptr, colidx, vals, X):
    """coupling_G, the product computed once per pattern and tiles (every split and both G0 modes share it)."""
    if key not in _COUPLING_REFS:
        _COUPLING_REFS[key] = A.coupling_G(None, rowptr, colidx, vals, X)
    G, mag = _COUPLING_REFS[key]
    return (G, mag) if G0 is None else (G + np.array(G0, dtype=A.LD), mag + np.abs(G0))


@pytest.mark.parametrize("d,r", DR)
def test_coupling_product_matches_longdouble_at_every_split(oracle, d, r):
    """G = G0 + Xnbr C through dpgo_problem_set_G_coupling + dpgo_problem_update_G_from_neighbors_device at DPGO_SPLIT = 1,
    2, 4 on n = 1, P - 1, P, P + 1, 17 P + 3 of EVERY split's tile P (so that the splits can be compared) and, per split,
    one n of more than 1 024 tiles (second trip of the tile walk); patterns (agent_layer_reference.coupling_pattern): rows
    without a block, the first and the last among them, a hub slot, rows of (d + 1) + 3 and 4 (d + 1) + 3 blocks; one
    column; no column (NULL tiles).  With G0 random and G0 = NULL.
    Rows without a block are G0 bit for bit; every other element is within (k + 2) 2^-53 (|G0| + |Xnbr| |C|) of the
    longdouble value, k = (d + 1) x blocks of the row: the forward error bound of a k-term fma sum in any order plus one
    addition.  The splits agree with each other to the same bound; a second update replaces G; dpgo_problem_set_G(NULL)
    takes G out of the product.  Largest error / bound per split: printed, and in every failure message."""
    import torch
    b = d + 1
    guard = guard_of(d, r)
    small = sorted({n for s in SPLITS for n in A.coupling_pose_counts(d, s)[:-1]})
    seen, worst = {}, {}
    for split in SPLITS:
        worst[split] = 0.0
        with library_options({"DPGO_SPLIT": str(split)}) as lib:
            big = A.coupling_pose_counts(d, split)[-1]
            for n in small + [big]:
                for kind in ("mixed",) if n == big else ("mixed", "one", "none"):
                    ncols = {"mixed": max(4 * b + 3, n // 3), "one": 1, "none": 0}[kind]
                    rowptr, colidx, vals, G0, X, info = _coupling_case(n, ncols, d, r, seed=1000 * n + ncols % 7)
                    X_d = [device_input(x, guard) if ncols else None for x in X]
                    h = Coupled(lib, _diag_Q(oracle, n, d), r, d, guard)
                    try:
                        assert "lane groups per pose %d;" % split in h.describe()
                        for g0 in (G0, None):
                            what = "d=%d r=%d split=%d n=%d %s G0=%s" % (d, r, split, n, kind, g0 is not None)
                            key = (n, kind, g0 is not None)
                            h.set_coupling(ncols, rowptr, colidx, vals, g0)
                            h.update(X_d[0])
                            first = h.G()
                            ref = _coupling_ref((d, r, n, kind, 0), g0, rowptr, colidx, vals, X[0])
                            worst[split] = max(worst[split], _check_G(first, ref, g0, rowptr, b, what))
                            if key in seen:  # the other splits: the same bound between them
                                bound = ((A.row_terms(rowptr, b) + 2) * A.U)[:, None, None] * ref[1]
                                diff = np.abs(np.array(first, dtype=A.LD) - seen[key])
                                assert np.all(diff <= bound), what + ": splits disagree"
                            else:
                                seen[key] = first
                            if n != big:  # another update replaces G: nothing of the first survives
                                h.update(X_d[1])
                                ref = _coupling_ref((d, r, n, kind, 1), g0, rowptr, colidx, vals, X[1])
                                worst[split] = max(worst[split], _check_G(h.G(), ref, g0, rowptr, b, what + " second"))
                        h.set_G(None)
                        assert not bits(h.G()).any(), what + ": G still added after set_G(NULL)"
                    except AssertionError as e:
                        raise AssertionError("%s (largest error / bound so far per split: %s)" % (e, worst)) from e
                    finally:
                        h.close()
                    del X_d
            torch.cuda.synchronize()
    _COUPLING_REFS.clear()
    print("coupling product d=%d r=%d: largest error / bound at split 1, 2, 4 = %s"
          % (d, r, ", ".join("%.3f" % worst[s] for s in SPLITS)))


def _ptrs(values):
    arr = (C.c_void_p * len(values))()
    for k, v in enumerate(values):
        arr[k] = v
    return arr


@pytest.mark.parametrize("d,r", [(3, 5), (2, 3), (3, 6)])
def test_entries_that_refresh_G_themselves(oracle, d, r):
    """dpgo_problem_eval_terms_device_many on three handles of different size, each with its own coupling operator and
    tiles: (XQX, X.G, |rgrad|^2) against the longdouble evaluation to the parity suite's scalar tolerance (1e-12 of the
    term's magnitude sum) and bit for bit the single-handle update + dpgo_problem_eval_terms_device on fresh handles; a
    handle whose tile pointer is NULL keeps its G while the others take new tiles.  dpgo_optimize_device_many (two RTR
    iterations of two tCG steps, multi-launch): fInit is that of a single solve after an explicit update, bit for bit."""
    import torch
    import dpgo_amd.lib as L
    b = d + 1
    guard = guard_of(d, r)
    P = tile_poses(d, 1)
    sizes = (P + 1, P - 1, 2 * P + 1)
    with library_options({}) as lib:
        cases, hs, fresh = [], [], []
        try:
            for k, n in enumerate(sizes):
                Qb, T = graph_Q(oracle, d, n)
                X = point(oracle, T, d, r, seed=n + r)[0]
                rowptr, colidx, vals, G0, Xn, _ = _coupling_case(n, max(4 * b + 3, n // 3), d, r, seed=50 + k)
                cases.append(dict(Q=Qb, X=X, C=(rowptr, colidx, vals), G0=G0, Xn=Xn, n=n,
                                  X_d=device_input(X, guard), Xn_d=[device_input(x, guard) for x in Xn]))
                for group in (hs, fresh):
                    h = Coupled(lib, Qb, r, d, guard)
                    group.append(h)
                    h.set_coupling(len(Xn[0]), rowptr, colidx, vals, G0)
                    L.check(lib.dpgo_problem_set_persistent(h.h, 0))
            handles = _ptrs([h.h.value for h in hs])
            xs = _ptrs([L.ptr(c["X_d"]) for c in cases])

            def many(which):
                out = np.full((3, 3), np.nan)
                nb = _ptrs([None if w is None else L.ptr(c["Xn_d"][w]) for c, w in zip(cases, which)])
                torch.cuda.synchronize()
                L.check(lib.dpgo_problem_eval_terms_device_many(3, handles, xs, nb, None, L.ptr(out)))
                return out

            def check(got, c, w, what):
                G, mag = A.coupling_G(c["G0"], *c["C"], c["Xn"][w])
                (xqx, xg, g2), (mq, mg) = A.eval_terms(c["Q"], G, mag, c["X"], d)
                assert abs(got[0] - xqx) <= 1e-12 * mq, (what, got[0], float(xqx))
                assert abs(got[1] - xg) <= 1e-12 * mg, (what, got[1], float(xg))
                assert abs(got[2] - g2) <= 1e-12 * g2, (what, got[2], float(g2))
                return float(0.5 * xqx + xg), float(0.5 * mq + mg)

            first = many([0, 0, 0])
            for k, c in enumerate(cases):
                check(first[k], c, 0, "handle %d" % k)
                fresh[k].update(c["Xn_d"][0])
                assert first[k].tolist() == list(fresh[k].eval_terms_device(c["X_d"])), k
            second = many([1, None, 1])
            assert same_bits(second[1], first[1])  # NULL tiles: the handle's G stays
            for k in (0, 2):
                check(second[k], cases[k], 1, "handle %d, second tiles" % k)
                assert not same_bits(second[k], first[k])
            # the solve entry: G from the tiles, then fInit
            cp = L.RoptParamsC()
            lib.dpgo_ropt_params_default(C.byref(cp))
            cp.RTR_iterations, cp.RTR_tCG_iterations = 2, 2
            its = [torch.from_numpy(c["X"].reshape(-1).copy()).to("cuda") for c in cases]
            res = (L.RoptResultC * 3)()
            torch.cuda.synchronize()
            L.check(lib.dpgo_optimize_device_many(3, handles, C.byref(cp), _ptrs([L.ptr(x) for x in its]),
                                                  _ptrs([L.ptr(c["Xn_d"][0]) for c in cases]), None, res))
            for k, c in enumerate(cases):
                f, fmag = check(first[k], c, 0, "handle %d" % k)
                assert abs(res[k].fInit - f) <= 1e-12 * fmag, (k, res[k].fInit, f)
                x = torch.from_numpy(c["X"].reshape(-1).copy()).to("cuda")
                one = L.RoptResultC()
                torch.cuda.synchronize()
                fresh[k].update(c["Xn_d"][0])
                L.check(lib.dpgo_optimize_device(fresh[k].h, C.byref(cp), L.ptr(x), C.byref(one)))
                assert res[k].fInit == one.fInit and res[k].gradNormInit == one.gradNormInit, (k, res[k].fInit, one.fInit)
        finally:
            for h in hs + fresh:
                h.close()


# ================================================================ C. relative change
@pytest.mark.parametrize("d,r", DR)
def test_relative_change_finds_the_maximum_wherever_it_sits(d, r):
    """dpgo_max_translation_distance_device at n = 1, 63, 64, 65, 255, 256, 257, 262 144 and 262 145 (the second grid-stride
    trip) with the maximum at pose 0, at the last pose, at lane 63 of the first wave and at the first pose of the second
    trip, every other distance at most half of it: within (r + 2) 2^-53 relative of the longdouble value (an r-term fma sum
    and a square root); out_dev == out_host bit for bit; the value does not depend on the rotation rows; X == Xprev gives
    exactly 0 into a word that held the previous, larger result."""
    import torch
    import dpgo_amd.lib as L
    lib = L.load()
    guard = guard_of(d, r)
    worst = 0.0

    def run(X_d, Xp_d, n):
        out, host = Guarded(1, 2, device=True), C.c_double(NAN)
        L.check(lib.dpgo_max_translation_distance_device(r, d, n, L.ptr(X_d), L.ptr(Xp_d), out.ptr(), C.byref(host), None))
        dev = out.result((1,))
        assert same_bits(dev, np.array([host.value]))
        return out, host.value

    for n in A.CHANGE_COUNTS:
        X, Xp = A.change_base(d, r, n, seed=n + 7 * r)
        X_d, Xp_d = device_input(X, guard), device_input(Xp, guard)
        Xp_v = Xp_d.view(n, d + 1, r)
        for place in A.CHANGE_PLACES:
            at = A.change_place(n, place)
            if at is None:
                continue
            keep = Xp[at, d, :].copy()
            Xp[at, d, :] = A.change_peak(X, at, seed=n + at)
            Xp_v[at, d, :] = torch.from_numpy(Xp[at, d, :]).to("cuda")
            torch.cuda.synchronize()
            want = A.max_translation_distance(X, Xp)
            assert abs(float(want) - 1.0) < 1e-12
            out, got = run(X_d, Xp_d, n)
            rel = float(abs(np.longdouble(got) - want) / want)
            worst = max(worst, rel / ((r + 2) * A.U))
            assert rel <= (r + 2) * A.U, (n, place, got, float(want), rel / A.U)
            if place in ("last", "second_trip"):
                # wild rotation rows, the same translations: the same bits
                X_d.view(n, d + 1, r)[:, :d, :].mul_(-3.7e5)
                Xp_v[:, :d, :].add_(1.0e3)
                torch.cuda.synchronize()
                assert run(X_d, Xp_d, n)[1] == got, (n, place)
                # no change at all: exactly 0, and the larger value the word held is gone
                host = C.c_double(NAN)
                L.check(lib.dpgo_max_translation_distance_device(r, d, n, L.ptr(X_d), L.ptr(X_d), out.ptr(), C.byref(host), None))
                assert not bits(out.result((1,))).any() and host.value == 0.0 and not np.signbit(host.value), (n, place)
            Xp[at, d, :] = keep
            Xp_v[at, d, :] = torch.from_numpy(keep).to("cuda")
        del X_d, Xp_d, Xp_v
    print("relative change d=%d r=%d: largest relative error / ((r + 2) 2^-53) = %.3f" % (d, r, worst))


# ================================================================ D. ordering words
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 70])
def test_flag_words_are_written_and_waited_for_table_by_table(n):
    """dpgo_flags_write_device on n words of one allocation (tables of kFlagCap = 32 words per launch): exactly those n
    words hold base + k afterwards and their neighbours are untouched.  dpgo_flags_wait_device_checked on the same stream,
    2 000 ms limit, pinned error word as dpgo_amd/ipc.py allocates its own: for the values just written, then for smaller
    ones; both return and the error word stays 0.  A null word anywhere in the table is refused before anything is
    launched: no word changes."""
    import torch
    import dpgo_amd.lib as L
    lib = L.load()
    pad, base, old = 3, 1000, 7
    words = torch.full((n + 2 * pad,), old, dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int64).pin_memory()
    torch.cuda.synchronize()
    ptrs = (C.c_void_p * max(n, 1))(*[words.data_ptr() + 8 * (pad + k) for k in range(n)])
    vals = (C.c_ulonglong * max(n, 1))(*[base + k for k in range(n)])
    L.check(lib.dpgo_flags_write_device(n, ptrs, vals, None))
    torch.cuda.synchronize()
    want = np.full(n + 2 * pad, old, dtype=np.int64)
    want[pad:pad + n] = base + np.arange(n)
    assert np.array_equal(words.cpu().numpy(), want)
    # every value waited for is already in place (written by the launch above, on the same stream)
    L.check(lib.dpgo_flags_wait_device_checked(n, ptrs, vals, 2000, C.c_void_p(err.data_ptr()), None))
    lower = (C.c_ulonglong * max(n, 1))(*[base + k - 1 - (k % 3) for k in range(n)])
    L.check(lib.dpgo_flags_wait_device_checked(n, ptrs, lower, 2000, C.c_void_p(err.data_ptr()), None))
    torch.cuda.synchronize()
    assert int(err[0].item()) == 0
    assert np.array_equal(words.cpu().numpy(), want)
    if n == 0:
        assert lib.dpgo_flags_write_device(0, None, None, None) == L.OK
        assert lib.dpgo_flags_wait_device_checked(0, None, None, 2000, C.c_void_p(err.data_ptr()), None) == L.OK
        return
    for hole in sorted({0, n - 1, n // 2}):  # (n = 70: word 35 belongs to the second table, word 69 to the third)
        holed = (C.c_void_p * n)(*[None if k == hole else ptrs[k] for k in range(n)])
        other = (C.c_ulonglong * n)(*[5 * base + k for k in range(n)])
        assert lib.dpgo_flags_write_device(n, holed, other, None) == L.ERR_INVALID, hole
        # (a wait that got as far as a launch would find its values in place: the words hold at least `lower`)
        assert lib.dpgo_flags_wait_device_checked(n, holed, lower, 2000, C.c_void_p(err.data_ptr()), None) == L.ERR_INVALID, hole
        torch.cuda.synchronize()
        assert np.array_equal(words.cpu().numpy(), want), "words written although the table was refused (null word %d)" % hole
    assert int(err[0].item()) == 0


# ================================================================ E. block-Jacobi factors
@pytest.mark.parametrize("d,r", [(2, 3), (3, 4)])
def test_block_jacobi_factors_against_longdouble_inverses(oracle, d, r):
    """k_build_dinv (Gauss-Jordan without pivoting, symmetrised) on the diagonal blocks of a pose graph whose edges carry
    kappa, tau in {1, 1e4, 1e8} and whose last pose has 60 edges more (agent_layer_reference.jacobi_graph), n = P + 1,
    shifts 0.1 and 1e-3.  The factors are read out through dpgo_problem_precondition: at a Stiefel point of signed
    coordinate axes, a V whose column j is one further axis passes block-Jacobi and the tangent projection as column j of
    Dinv_i, bit for bit (every other product is an exact zero).  Dinv is symmetric; per conditioning class its error against
    the longdouble inverse is at most 32 times that of np.linalg.inv on the same blocks (both numbers in the message);
    every Dinv_i is positive definite."""
    import dpgo_amd.lib as L
    b = d + 1
    n = tile_poses(d, 1) + 1
    guard = guard_of(d, r)
    rowptr, colidx, vals, diag = jacobi_bsr(d, n)
    X, axis = A.axis_frames(d, r, n, seed=3)
    report = []
    with library_options({}) as lib:
        h = Handle(lib, oracle.BSR(n, b, rowptr, colidx, vals), r, d)
        try:
            for shift in (0.1, 1e-3):
                blocks = diag + shift * np.eye(b)
                Dinv = np.empty((n, b, b))
                for j in range(b):
                    V = np.zeros((n, b, r))
                    V[np.arange(n), j, axis] = 1.0
                    o = h.out(guard)
                    L.check(lib.dpgo_problem_precondition(h.h, L.PRECOND_BLOCK_JACOBI, shift, L.ptr(X), L.ptr(V), o.ptr()))
                    Z = o.result((n, b, r))
                    Dinv[:, :, j] = Z[np.arange(n), :, axis]
                    Z[np.arange(n), :, axis] = 0.0
                    assert not Z.any(), "the read-out is not exact"
                assert same_bits(Dinv, np.ascontiguousarray(np.swapaxes(Dinv, 1, 2))), "Dinv is not symmetric"
                exact = A.block_inverse(blocks)
                dev = A.inverse_error(Dinv, exact)
                ref = A.inverse_error(np.linalg.inv(blocks), exact)
                cls, k2 = A.condition_class(blocks)
                for c in range(3):
                    line = "d=%d shift=%g class %d (kappa_2 %.1e .. %.1e, %d poses): device %.3e, numpy %.3e" % (
                        d, shift, c, k2[cls == c].min(), k2[cls == c].max(), int(np.sum(cls == c)), dev[cls == c].max(),
                        ref[cls == c].max())
                    report.append(line)
                    assert dev[cls == c].max() <= 32 * ref[cls == c].max(), line
                lam = np.linalg.eigvalsh(Dinv)[:, 0]
                assert np.all(lam > 0), (shift, int(np.argmin(lam)), float(lam.min()))
        finally:
            h.close()
    print("\n".join(report))
