"""GPU: guided descriptor matching (vo_match_guided_hamming / vo_match_guided_l2, csrc/vo_match.hip) against its numpy definition
tests/gmatch_model.py -- match, idx, dist, n_admitted and rbest for equality, no tolerances -- at the smallest shapes at which the kernels can
go wrong, the properties that hold by construction, and one pass over real ORB descriptors.  The plain matchers (vo_match_knn2 /
vo_match_hamming_knn2) are the same scans at gate 0 on the same workspace: they are held to the model here as well."""
import ctypes as C

import numpy as np
import pytest

import fundamental_model as fm
import gmatch_cases as gc
import gmatch_model as gm
from test_gmatch_model import check_property_a, mutual_pairs

pytestmark = pytest.mark.gpu

KEYS = ("match", "idx", "dist", "n_admitted", "rbest")
HAM_TILE_ROWS = {4: 1024, 32: 1024, 64: 542}            # min(1024 staged positions, 9216 words / (nbytes / 4 + 1)) rows per LDS tile under a gate
HAM_TILE_ROWS_GATE_0 = {4: 4608}                        # gate 0 stages no positions: 9216 words / (nbytes / 4 + 1)


@pytest.fixture(scope="module")
def ctx():
    from vo_mi355x import VoContext
    with VoContext(64, 64, max_pts=64) as c:
        yield c


def _same(got, want, what=""):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, got[k], want[k])


def _check(c, d1, d2, **kw):
    got = c.match_guided(d1, d2, **kw)
    want = gm.match_guided(d1, d2, **kw)
    _same(got, want, {k: v for k, v in kw.items() if np.ndim(v) == 0})
    return got, want


def _all_gates(c, d1, d2, seed, share=0.5):
    n1, n2 = len(d1), len(d2)
    p1, p2 = gc.positions(n1, n2, seed)
    for gate in (0, 1, 2, 3):
        kw = gc.gate_kwargs(gate, share, p1, p2, F=gc.F_FORWARD if gate == 3 else gc.F_GENERAL)
        _check(c, d1, d2, **kw)
        _check(c, d1, d2, ratio=0.9, cross_check=True, **kw)


@pytest.mark.parametrize("nbytes", [4, 32, 64])
@pytest.mark.parametrize("n2", [1, 63, 65, "tile+1"])
def test_hamming_shapes(ctx, nbytes, n2):
    n2 = HAM_TILE_ROWS[nbytes] + 1 if n2 == "tile+1" else n2
    for n1 in (1, 5, 9):
        d1, d2 = gc.hamming_sets(n1, n2, nbytes, 1)
        _all_gates(ctx, d1, d2, n1)


def test_hamming_gate_0_beyond_one_tile_of_four_byte_rows(ctx):
    """the ungated instance's tile is not cut at the 1024 staged positions: at nbytes = 4 a second tile begins at row 4608"""
    d1, d2 = gc.hamming_sets(5, HAM_TILE_ROWS_GATE_0[4] + 1, 4, 1)
    d2[-1] = d1[3]                                                      # the one row of the second tile is query 3's nearest
    got, _ = _check(ctx, d1, d2)
    assert got["idx"][3, 0] == len(d2) - 1 and got["dist"][3, 0] == 0 and (got["n_admitted"] == len(d2)).all()


@pytest.mark.parametrize("dim", [6, 128])
@pytest.mark.parametrize("n2", [1, 65, 200])
@pytest.mark.parametrize("integer", [False, True])
def test_l2_shapes(ctx, dim, n2, integer):
    for n1 in (1, 5, 9):
        d1, d2 = gc.l2_sets(n1, n2, dim, 2, integer)
        _all_gates(ctx, d1, d2, n1)


def _sets(ham, n1, n2, seed):
    return gc.hamming_sets(n1, n2, 32, seed) if ham else gc.l2_sets(n1, n2, 32, seed, integer=True)


@pytest.mark.parametrize("ham", [True, False])
@pytest.mark.parametrize("gate,share", [(1, 0.05), (1, 0.5), (2, 0.05), (2, 0.5), (3, 0.05), (3, 0.5)])
def test_gates_at_two_shares_with_edge_rows(ctx, ham, gate, share):
    n1, n2 = 70, 150
    d1, d2 = _sets(ham, n1, n2, 30 + gate)
    p1, p2 = gc.positions(n1, n2, 30 + gate)
    F = gc.F_FORWARD if gate == 3 else gc.F_GENERAL
    p2 = gc.true_positions(gate, F, p1, p2, 30)
    kw = gc.gate_kwargs(gate, share, p1, p2, F=F)                       # the gate distances of the ordinary rows
    NONE, LONE, LONE_T, NAN_Q, NAN_T = 66, 67, 140, 68, 141
    p1, p2 = gc.plant_edges(p1, p2, gate, F, lone_q=LONE, lone_t=LONE_T, none_q=NONE, nan_q=NAN_Q, nan_t=NAN_T)
    kw.update(pts1=p1, pts2=p2)
    for ratio, max_dist, cross in ((0.8, None, False), (1.0, None, True), (0.9, 90.0 if ham else 400.0, True)):
        got, want = _check(ctx, d1, d2, ratio=ratio, max_dist=max_dist, cross_check=cross, **kw)
    print("gate %d target %.2f: admitted share %.4f, accepted %d of %d" % (gate, share, want["admitted"].mean(), (got["match"] >= 0).sum(), n1))
    got, _ = _check(ctx, d1, d2, ratio=0.8, **kw)
    assert got["n_admitted"][NONE] == 0 and got["match"][NONE] == -1 and list(got["idx"][NONE]) == [-1, -1]      # no admitted row
    assert got["n_admitted"][NAN_Q] == 0 and got["match"][NAN_Q] == -1                                         # a NaN query position
    assert not (got["idx"] == NAN_T).any()                                                                     # a NaN train position
    # exactly one admitted row: the ratio test passes, the second slot is empty
    assert got["n_admitted"][LONE] == 1 and list(got["idx"][LONE]) == [LONE_T, -1] and got["match"][LONE] == LONE_T
    assert got["dist"][LONE, 1] == (gm.INT_MAX if ham else np.inf)


@pytest.mark.parametrize("ham", [True, False])
def test_window_centres_differ_from_the_query_positions(ctx, ham):
    """centers: the forward pass compares pts2 with the centres, the epipolar gate still reads pts1; the reverse pass stages both"""
    n1, n2 = 40, 90
    d1, d2 = _sets(ham, n1, n2, 8)
    p1, p2 = gc.positions(n1, n2, 8)
    ce = (p1 + np.float32(7.5)).astype(np.float32)
    for gate in (1, 3):
        kw = gc.gate_kwargs(gate, 0.3, p1, p2, F=gc.F_FORWARD, centers=ce)
        got, _ = _check(ctx, d1, d2, cross_check=True, **kw)
        other = ctx.match_guided(d1, d2, cross_check=True, **{k: v for k, v in kw.items() if k != "centers"})
        assert not np.array_equal(got["n_admitted"], other["n_admitted"])


@pytest.mark.parametrize("ham", [True, False])
def test_a_degenerate_epipolar_line_admits_nothing(ctx, ham):
    """under F_FORWARD the epipolar line of (0, 0) has a^2 + b^2 = 0 in either view: 0 * inf = NaN, never admitted"""
    n1, n2 = 20, 70
    d1, d2 = _sets(ham, n1, n2, 9)
    p1, p2 = gc.positions(n1, n2, 9)
    p1[4] = 0.0; p2[66] = 0.0
    d2[66] = d1[4]                                                      # ... although their descriptors agree
    kw = gc.gate_kwargs(2, 0.5, p1, p2, F=gc.F_FORWARD)
    got, want = _check(ctx, d1, d2, cross_check=True, **kw)
    assert got["n_admitted"][4] == 0 and got["match"][4] == -1 and got["rbest"][66] == -1 and not (got["idx"] == 66).any()
    assert not want["admitted"][4].any() and not want["admitted"][:, 66].any() and want["admitted"].any()


@pytest.mark.parametrize("ham", [True, False])
def test_ties(ctx, ham):
    n1, n2 = 12, 80
    d1, d2 = _sets(ham, n1, n2, 10)
    d2[70] = d2[33] = d2[10] = d1[0]                                    # three copies of query 0 among the train rows: the lowest two win
    d1[7] = d1[3]; d2[5] = d1[3]                                        # queries 3 and 7 are equal, train row 5 is their copy
    p1, p2 = gc.positions(n1, n2, 10)
    for kw in ({}, dict(pts1=p1, pts2=p2, radius=1000.0)):
        got, _ = _check(ctx, d1, d2, cross_check=True, **kw)
        assert list(got["idx"][0]) == [10, 33] and got["dist"][0, 0] == 0 and got["dist"][0, 1] == 0 and got["match"][0] == 10
        assert got["idx"][3, 0] == 5 and got["idx"][7, 0] == 5 and got["rbest"][5] == 3
        assert got["match"][3] == 5 and got["match"][7] == -1           # only the lower query keeps the match
    p2[10] = np.nan                                                     # gated out: the next copies move up
    got, _ = _check(ctx, d1, d2, pts1=p1, pts2=p2, radius=1000.0)
    assert list(got["idx"][0]) == [33, 70]


def _plain_is_the_model(idx, dist, d1, d2, what=""):
    want = gm.match_guided(d1, d2)
    assert idx.dtype == want["idx"].dtype and np.array_equal(idx, want["idx"]), (what, idx, want["idx"])
    assert dist.dtype == want["dist"].dtype and np.array_equal(dist, want["dist"]), (what, dist, want["dist"])


def test_gate_0_is_the_plain_matcher_bit_for_bit(ctx):
    rng = np.random.default_rng(12)
    for dim, n1, n2 in ((128, 130, 300), (6, 9, 70)):
        d1 = rng.standard_normal((n1, dim)).astype(np.float32) * 40; d2 = rng.standard_normal((n2, dim)).astype(np.float32) * 40
        d2[3] = d2[90 % n2]
        idx, dist = ctx.match_knn2(d1, d2)
        got = ctx.match_guided(d1, d2)
        assert np.array_equal(got["idx"], idx) and np.array_equal(got["dist"].view(np.uint32), dist.view(np.uint32))
        assert np.array_equal(got["match"], idx[:, 0]) and (got["n_admitted"] == n2).all()
        _plain_is_the_model(idx, dist, d1, d2)                          # both sides run one kernel: the model is the independent pin
    for nb, n1, n2 in ((32, 130, 1100), (4, 9, 70)):
        d1 = rng.integers(0, 256, (n1, nb), dtype=np.uint8); d2 = rng.integers(0, 256, (n2, nb), dtype=np.uint8)
        idx, dist = ctx.match_hamming_knn2(d1, d2)
        got = ctx.match_guided(d1, d2)
        assert np.array_equal(got["idx"], idx) and np.array_equal(got["dist"], dist) and got["dist"].dtype == dist.dtype
        _plain_is_the_model(idx, dist, d1, d2)


@pytest.mark.parametrize("ham", [True, False])
def test_batch_of_three_with_counts(ctx, ham):
    from vo_mi355x import VoContext
    n1, n2 = 9, 70
    sets = [_sets(ham, n1, n2, 40 + b) for b in range(3)]
    pos = [gc.positions(n1, n2, 40 + b) for b in range(3)]
    d1, d2 = np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets])
    p1, p2 = np.stack([p[0] for p in pos]), np.stack([p[1] for p in pos])
    Fs = np.stack([gc.F_FORWARD, gc.F_GENERAL, gc.F_FORWARD.T])
    with VoContext(64, 64, max_pts=64, batch=3) as cb:
        for counts1, counts2 in (((9, 0, 5), (66, 70, 1)), ((3, 9, 9), (70, 65, 0)), (None, (64, 0, 70))):
            for kw in (dict(), dict(radius=40.0), dict(radius=60.0, epi_dist=25.0)):
                if "epi_dist" in kw:
                    kw["F"] = Fs
                if kw:
                    kw.update(pts1=p1, pts2=p2)
                got = cb.match_guided(d1, d2, cross_check=True, ratio=0.9, counts1=counts1, counts2=counts2, **kw)
                for b in range(3):
                    kb = {k: (v[b] if np.ndim(v) > 0 else v) for k, v in kw.items()}
                    c1 = None if counts1 is None else counts1[b]
                    one = ctx.match_guided(d1[b], d2[b], cross_check=True, ratio=0.9, counts1=c1, counts2=counts2[b], **kb)
                    want = gm.match_guided(d1[b], d2[b], cross_check=True, ratio=0.9, count1=c1, count2=counts2[b], **kb)
                    _same({k: got[k][b] for k in KEYS}, want, ("batched", b))
                    _same(one, want, ("single", b))
                    if c1 == 0 or counts2[b] == 0:
                        assert (want["match"] == -1).all() and (want["idx"] == -1).all() and (want["rbest"] == -1).all()


@pytest.mark.parametrize("ham", [True, False])
def test_the_workspace_grows_then_shrinks(ham):
    from vo_mi355x import VoContext
    with VoContext(64, 64, max_pts=64) as c:
        for n1, n2 in ((5, 9), (70, 300), (5, 9), (3, 400)):
            d1, d2 = _sets(ham, n1, n2, n1 + n2)
            p1, p2 = gc.positions(n1, n2, n1 + n2)
            _check(c, d1, d2, cross_check=True, ratio=0.9, **gc.gate_kwargs(3, 0.5, p1, p2, F=gc.F_FORWARD))
            _check(c, d1, d2)


def test_the_four_entry_points_share_one_workspace():
    """one context, batch 2: the plain and the guided calls of both kinds take turns over sets that grow, shrink and grow on one side only,
    at two row widths each.  A buffer sized by one kind and read by another, or a capacity left stale by a smaller call, would show."""
    from vo_mi355x import VoContext
    Fs = np.stack([gc.F_FORWARD, gc.F_GENERAL])
    with VoContext(64, 64, max_pts=64, batch=2) as c:
        for n1, n2 in ((5, 9), (70, 300), (5, 9), (3, 400)):
            for dim, nbytes in ((6, 32), (128, 4)):
                fs = [gc.l2_sets(n1, n2, dim, 60 + b, integer=False) for b in range(2)]
                hs = [gc.hamming_sets(n1, n2, nbytes, 60 + b) for b in range(2)]
                pos = [gc.positions(n1, n2, 60 + b) for b in range(2)]
                f1, f2, h1, h2, p1, p2 = (np.stack([x[k] for x in xs]) for xs in (fs, hs, pos) for k in (0, 1))
                kw = dict(pts1=p1, pts2=p2, radius=60.0, epi_dist=25.0, F=Fs, cross_check=True, ratio=0.9)
                for d1, d2, plain in ((f1, f2, c.match_knn2), (h1, h2, c.match_hamming_knn2)):
                    idx, dist = plain(d1, d2)
                    guided = c.match_guided(d1, d2, **kw)
                    for b in range(2):
                        what = (n1, n2, d1.shape[-1], str(d1.dtype), b)
                        _plain_is_the_model(idx[b], dist[b], d1[b], d2[b], what)
                        _same({k: guided[k][b] for k in KEYS}, gm.match_guided(d1[b], d2[b], **{k: (v[b] if np.ndim(v) > 0 else v) for k, v in kw.items()}), what)


def _raw(c, ham, **over):
    """one raw call with valid arguments, then `over` applied -> (rc, outputs untouched?)"""
    from vo_mi355x import _lib
    n1, n2, wd = 5, 9, (8 if ham else 6)
    d1, d2 = gc.hamming_sets(n1, n2, wd, 1) if ham else gc.l2_sets(n1, n2, wd, 1, False)
    p1, p2 = gc.positions(n1, n2, 1)
    a = dict(desc1=d1, n1=n1, desc2=d2, n2=n2, width=wd, pts1=p1, pts2=p2, centers=p1.copy(), F=np.ascontiguousarray(gc.F_GENERAL),
             counts1=np.array([n1], np.int32), counts2=np.array([n2], np.int32), gate=3, cross_check=1, radius=30.0, epi_dist=20.0, ratio=0.8,
             max_dist=1e9, match=np.full(n1, 77, np.int32), idx=np.full((n1, 2), 77, np.int32),
             dist=np.full((n1, 2), 77, np.int32 if ham else np.float32), n_admitted=np.full(n1, 77, np.int32), rbest=np.full(n2, 77, np.int32))
    a.update(over)
    prm = _lib.GMatchParams(gate=a["gate"], cross_check=a["cross_check"], radius=a["radius"], epi_dist=a["epi_dist"], ratio=a["ratio"],
                            max_dist=a["max_dist"])
    dt, ot = (C.c_uint8, C.c_int32) if ham else (C.c_float, C.c_float)
    fn = c._L.vo_match_guided_hamming if ham else c._L.vo_match_guided_l2
    ptr = _lib.ptr
    rc = fn(c._h, ptr(a["desc1"], dt), a["n1"], ptr(a["desc2"], dt), a["n2"], a["width"], ptr(a["pts1"], C.c_float), ptr(a["pts2"], C.c_float),
            ptr(a["centers"], C.c_float), ptr(a["F"], C.c_double), ptr(a["counts1"], C.c_int32), ptr(a["counts2"], C.c_int32), C.byref(prm),
            ptr(a["match"], C.c_int32), ptr(a["idx"], C.c_int32), ptr(a["dist"], ot), ptr(a["n_admitted"], C.c_int32), ptr(a["rbest"], C.c_int32))
    untouched = all(a[k] is None or (a[k] == 77).all() for k in ("match", "idx", "dist", "n_admitted", "rbest"))
    return rc, untouched


INVALID = [dict(desc1=None), dict(desc2=None), dict(match=None), dict(n1=0), dict(n2=0), dict(n1=-3),
           dict(gate=-1), dict(gate=4), dict(cross_check=-1), dict(cross_check=2),
           dict(radius=0.0), dict(radius=-1.0), dict(radius=np.inf), dict(radius=np.nan),
           dict(epi_dist=0.0), dict(epi_dist=-1.0), dict(epi_dist=np.inf), dict(epi_dist=np.nan),
           dict(pts1=None), dict(pts2=None), dict(gate=1, pts1=None), dict(gate=2, pts2=None), dict(F=None), dict(gate=2, F=None),
           dict(ratio=0.0), dict(ratio=-0.5), dict(ratio=1.5), dict(ratio=np.nan), dict(max_dist=np.nan), dict(max_dist=-1.0),
           dict(counts1=np.array([-1], np.int32)), dict(counts1=np.array([6], np.int32)),
           dict(counts2=np.array([-1], np.int32)), dict(counts2=np.array([10], np.int32))]


@pytest.mark.parametrize("ham", [True, False])
def test_invalid_arguments_leave_the_outputs_untouched(ctx, ham):
    rc, untouched = _raw(ctx, ham)
    assert rc == 0 and not untouched                                    # the valid call the cases below are one step away from
    widths = (0, 2, 6, 68, -4) if ham else (0, -1)
    for over in INVALID + [dict(width=w) for w in widths]:
        rc, untouched = _raw(ctx, ham, **over)
        assert rc == -1 and untouched, over
    # what is valid: no optional output, no centres, no F without the epipolar gate, a radius nobody reads, a count of 0
    for over in (dict(idx=None, dist=None, n_admitted=None, rbest=None), dict(centers=None), dict(gate=1, F=None), dict(gate=0, radius=-1.0, epi_dist=np.nan),
                 dict(gate=0, pts1=None, pts2=None, F=None, centers=None), dict(counts1=np.array([0], np.int32)), dict(counts1=None, counts2=None),
                 dict(ratio=1.0, max_dist=np.inf), dict(max_dist=0.0)):
        rc, _ = _raw(ctx, ham, **over)
        assert rc == 0, over


@pytest.mark.parametrize("ham", [True, False])
@pytest.mark.parametrize("gate,share", [(1, 0.05), (2, 0.5), (3, 0.05)])
def test_properties_a_and_b(ctx, ham, gate, share):
    n1, n2 = 60, 80
    d1, d2 = gc.hamming_sets(n1, n2, 8, 21) if ham else gc.l2_sets(n1, n2, 16, 21, integer=True)
    d2[40:50] = d2[0:10]                                                # repeated texture
    p1, p2 = gc.positions(n1, n2, 21)
    F = gc.F_FORWARD if gate == 3 else gc.F_GENERAL
    p2 = gc.true_positions(gate, F, p1, p2, 30)
    kw = gc.gate_kwargs(gate, share, p1, p2, F=F)
    admitted = gm.admitted(n1, n2, p1, p2, kw.get("F"), None, kw.get("radius"), kw.get("epi_dist"))
    for ratio in (0.8, 1.0):
        plain = ctx.match_guided(d1, d2, ratio=ratio)
        guided = ctx.match_guided(d1, d2, ratio=ratio, **kw)
        a = check_property_a(plain, guided, admitted)
        print("gate %d share %.3f ratio %.1f (a) plain accepted %d, of them admitted %d, of them guided matches %d; guided accepted %d"
              % ((gate, admitted.mean(), ratio) + a + ((guided["match"] >= 0).sum(),)))
        assert a[1] == a[2]
    plain = ctx.match_guided(d1, d2, cross_check=True)
    guided = ctx.match_guided(d1, d2, cross_check=True, **kw)
    pairs = [(i, j) for i, j in mutual_pairs(plain) if admitted[i, j]]
    kept = [(i, j) for i, j in pairs if guided["match"][i] == j]
    print("(b) mutual-nearest pairs of the plain search %d, of them admitted %d, of them guided matches %d" % (len(mutual_pairs(plain)), len(pairs), len(kept)))
    assert kept == pairs


@pytest.mark.parametrize("t", [1.0, 3.0])
def test_property_c_inliers_of_the_search_are_admitted(ctx, t):
    """the raw call: F0 at unit norm, as the search counted its consensus.  Train row i carries query i's descriptor and no other row does, so
    idx[i][0] == i exactly where the gate admits the pair (i, i)"""
    from vo_mi355x import _lib
    s = fm.with_outliers("general", 200, 0.4, 3)
    p1, p2 = np.ascontiguousarray(s["p1"], np.float32), np.ascontiguousarray(s["p2"], np.float32)
    n = len(p1)
    prm = _lib.FundParams()
    ctx._L.vo_fundamental_default_params(C.byref(prm))
    prm.threshold, prm.seed = t, fm.SEARCH_SEED
    F, F0, mask = np.zeros(9), np.zeros(9), np.zeros(n, np.uint8)
    st = (_lib.FundStats * 1)()
    assert ctx._L.vo_fundamental_ransac(ctx._h, _lib.ptr(p1, C.c_float), _lib.ptr(p2, C.c_float), n, C.byref(prm), _lib.ptr(F, C.c_double),
                                        _lib.ptr(F0, C.c_double), _lib.ptr(mask, C.c_uint8), st) == 0 and st[0].status == 0
    d = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4).copy()
    got, _ = _check(ctx, d, d, pts1=p1, pts2=p2, F=F0.reshape(3, 3), epi_dist=t, cross_check=True)
    own = got["idx"][:, 0] == np.arange(n)
    print("threshold %.1f: %d inliers of %d, all admitted: %s; pairs (i, i) admitted %d" % (t, mask.sum(), n, own[mask != 0].all(), own.sum()))
    assert mask.sum() >= 7 and own[mask != 0].all()
    assert np.array_equal(own, mask != 0)                               # the same function: admitted exactly where the search saw an inlier


def test_end_to_end_on_orb_descriptors():
    """frames 0 and 4 of the sway scene at its default size: ORB, plain Hamming match with a mutual-nearest filter, fundamental matrix, guided
    match with cross-check under that F.  The counts are reported, not asserted."""
    from vo_mi355x import VoContext, synthetic as syn
    sc = syn.sway_scene(5)
    h, w = sc["frames"][0].shape
    t = 3.0
    with VoContext(w, h, max_pts=64) as c:
        (k0, d0), (k4, d4) = c.orb_detect_compute(sc["frames"][0]), c.orb_detect_compute(sc["frames"][4])
        p0, p4 = (np.ascontiguousarray(np.stack([k["x"], k["y"]], 1), np.float32) for k in (k0, k4))
        assert len(p0) >= 50 and len(p4) >= 50, (len(p0), len(p4))
        plain = c.match_guided(d0, d4, cross_check=True)                                   # gate 0: the plain search ...
        idx, _ = c.match_hamming_knn2(d0, d4); ridx, _ = c.match_hamming_knn2(d4, d0)
        mutual = [(i, int(idx[i, 0])) for i in range(len(d0)) if ridx[idx[i, 0], 0] == i]    # ... and the Python mutual-nearest filter
        assert mutual == mutual_pairs(plain)
        q, tr = np.array([m[0] for m in mutual]), np.array([m[1] for m in mutual])
        F, inl, st, _F0 = c.find_fundamental(p0[q], p4[tr], threshold=t, seed=1)
        assert st["status"] == 0
        guided = c.match_guided(d0, d4, pts1=p0, pts2=p4, F=F, epi_dist=t, cross_check=True)
    want = gm.match_guided(d0, d4, pts1=p0, pts2=p4, F=F, epi_dist=t, cross_check=True)
    _same(guided, want)
    admitted = gm.epi_admitted(F, p0, p4, t)
    pairs = [(i, j) for i, j in mutual if admitted[i, j]]
    assert all(guided["match"][i] == j for i, j in pairs)                                  # property (b) on real descriptors
    gmatches = mutual_pairs(guided)
    assert all(admitted[i, j] for i, j in gmatches)                                        # every guided match satisfies the gate under F

    def correct(ms):
        if not ms:
            return 0
        a, b = np.array([m[0] for m in ms]), np.array([m[1] for m in ms])
        return int((np.linalg.norm(sc["surface"](4, p4[b])[1] - p0[a], axis=1) <= 2.0).sum())
    print("ORB keypoints %d / %d; admitted share %.4f" % (len(p0), len(p4), admitted.mean()))
    print("plain mutual-nearest: %d matches, %d within 2 px of the truth" % (len(mutual), correct(mutual)))
    print("RANSAC inliers at %.1f px: %d, %d within 2 px" % (t, len(inl), correct([mutual[k] for k in inl])))
    print("guided (epi_dist %.1f, cross-check): %d matches, %d within 2 px; of the %d plain ones %d are admitted and all kept"
          % (t, len(gmatches), correct(gmatches), len(mutual), len(pairs)))


@pytest.mark.parametrize("ham", [True, False])
def test_extractor_match_guided_over_objects_with_uv_and_des(ctx, ham):
    """Extractor.match_guided: descriptor rows and positions gathered from `.des` and `.uv`, the accepted queries returned as DMatch"""
    from types import SimpleNamespace
    from vo_mi355x.extractor import Extractor
    n1, n2 = 30, 70
    d1, d2 = _sets(ham, n1, n2, 50)
    p1, p2 = gc.positions(n1, n2, 50)
    p2 = gc.true_positions(3, gc.F_FORWARD, p1, p2, 15)
    l1 = [SimpleNamespace(uv=p1[i].reshape(2, 1), des=d1[i].reshape(-1, 1)) for i in range(n1)]
    l2 = [SimpleNamespace(uv=p2[j].reshape(2, 1), des=d2[j].reshape(-1, 1)) for j in range(n2)]
    ce = (p1 * np.float32(1.01)).astype(np.float32)
    ext = Extractor(ctx=ctx)
    for kw in (dict(ratio=0.8), dict(F=gc.F_FORWARD, epi_dist=2.0, cross_check=True), dict(centers=ce, radius=5.0, ratio=0.9),
               dict(F=gc.F_FORWARD, epi_dist=2.0, centers=ce, radius=20.0, max_dist=60.0 if ham else 300.0)):
        got = ext.match_guided(l1, l2, **kw)
        want = gm.match_guided(d1, d2, pts1=p1, pts2=p2, **kw)
        acc = np.nonzero(want["match"] >= 0)[0]
        assert len(acc) > 0 and [(m.queryIdx, m.trainIdx, m.distance) for m in got] == [(i, want["match"][i], float(want["dist"][i, 0])) for i in acc]
    assert ext.match_guided([], l2) == [] and ext.match_guided(l1, []) == []


@pytest.mark.parametrize("share", [0.05, 0.5])
def test_l2_beyond_one_position_tile_and_around_the_ring(ctx, share):
    """n2 = 1100: a second tile of 1024 staged positions; admitted rows enter the wave's ring of 128 at offsets that are no multiple of 64 and
    wrap it several times"""
    d1, d2 = gc.l2_sets(5, 1100, 6, 7, integer=False)
    _all_gates(ctx, d1, d2, 7, share=share)
