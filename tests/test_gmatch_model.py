"""CPU-only: the numpy definition of guided matching (tests/gmatch_model.py) against triple Python loops on tiny sets, against the matcher
oracle where no gate and no rule is set, its epipolar predicate against the fundamental-matrix model's consensus test, and the two properties
that hold by construction."""
import math

import numpy as np
import pytest

import fundamental_model as fm
import gmatch_cases as gc
import gmatch_model as gm


def _loops(d1, d2, p1, p2, ce, F, radius, epi, ratio, max_dist, cross):
    """scalar restatement: one pair at a time, Python floats (float64) throughout"""
    n1, n2 = len(d1), len(d2)
    ham = d1.dtype == np.uint8
    adm = [[True] * n2 for _ in range(n1)]
    D = [[None] * n2 for _ in range(n1)]
    for i in range(n1):
        for j in range(n2):
            ok = True
            if radius is not None:
                c = p1[i] if ce is None else ce[i]
                dx, dy = float(p2[j][0]) - float(c[0]), float(p2[j][1]) - float(c[1])
                ok = ok and (dx * dx + dy * dy) <= radius * radius
            if epi is not None:
                f = [float(v) for v in np.asarray(F).reshape(9)]
                x, y, u, v = float(p1[i][0]), float(p1[i][1]), float(p2[j][0]), float(p2[j][1])
                a2, b2, c2 = (f[0] * x + f[1] * y) + f[2], (f[3] * x + f[4] * y) + f[5], (f[6] * x + f[7] * y) + f[8]
                a1, b1, c1 = (f[0] * u + f[3] * v) + f[6], (f[1] * u + f[4] * v) + f[7], (f[2] * u + f[5] * v) + f[8]
                g2, g1 = a2 * a2 + b2 * b2, a1 * a1 + b1 * b1
                if g1 == 0 or g2 == 0:
                    ok = False
                else:
                    d2_, d1_ = (u * a2 + v * b2) + c2, (x * a1 + y * b1) + c1
                    e1, e2 = (d1_ * d1_) * (1.0 / g1), (d2_ * d2_) * (1.0 / g2)
                    ok = ok and e1 <= epi * epi and e2 <= epi * epi
            adm[i][j] = bool(ok)
            if ham:
                D[i][j] = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(d1[i], d2[j]))
            else:
                acc = 0.0
                for k in range(d1.shape[1]):
                    e = float(d1[i][k]) - float(d2[j][k])
                    acc += e * e
                D[i][j] = float(np.sqrt(np.float32(acc)))

    def best(rows, cols, dist):
        out = []
        for r in rows:
            c = sorted((dist(r, k), k) for k in cols if adm_rc(r, k) and not math.isnan(dist(r, k)))
            out.append(c[:2])
        return out
    adm_rc = lambda i, j: adm[i][j]                                    # noqa: E731
    fwd = best(range(n1), range(n2), lambda i, j: D[i][j])
    adm_rc = lambda j, i: adm[i][j]                                    # noqa: E731
    rev = best(range(n2), range(n1), lambda j, i: D[i][j])
    rbest = [(r[0][1] if r else -1) if cross else -1 for r in rev]
    match = []
    for i, c in enumerate(fwd):
        ok = bool(c) and c[0][0] <= (math.inf if max_dist is None else max_dist)
        ok = ok and (ratio == 1.0 or len(c) < 2 or c[0][0] < ratio * c[1][0])
        ok = ok and (not cross or rbest[c[0][1]] == i)
        match.append(c[0][1] if ok else -1)
    return match, fwd, [sum(r) for r in adm], rbest


@pytest.mark.parametrize("ham", [True, False])
@pytest.mark.parametrize("gate", [0, 1, 2, 3])
def test_model_equals_scalar_loops(ham, gate):
    n1, n2 = 7, 9
    d1, d2 = gc.hamming_sets(n1, n2, 4, 3) if ham else gc.l2_sets(n1, n2, 6, 3, integer=False)
    d2[5] = d2[2]; d1[4] = d1[1]                                        # repeated rows on both sides
    p1, p2 = gc.positions(n1, n2, 3)
    F = gc.F_FORWARD if gate == 3 else gc.F_GENERAL
    kw = gc.gate_kwargs(gate, 0.5, p1, p2, F=F)                         # the gate distances of the ordinary rows
    p1, p2 = gc.plant_edges(p1, p2, gate, F, lone_q=2, lone_t=3, none_q=5, nan_q=6, nan_t=8)
    ce = p1 + np.float32(3.0) if gate & 1 else None
    if ce is not None:
        ce[2] = p1[2]
        kw.update(centers=ce)
    if gate:
        kw.update(pts1=p1, pts2=p2)
    for ratio, max_dist, cross in ((1.0, None, False), (0.8, None, False), (1.0, None, True), (0.9, 12.0 if ham else 3.0, True)):
        got = gm.match_guided(d1, d2, ratio=ratio, max_dist=max_dist, cross_check=cross, **kw)
        match, fwd, nadm, rbest = _loops(d1, d2, p1, p2, ce, kw.get("F"), kw.get("radius"), kw.get("epi_dist"), ratio, max_dist, cross)
        assert list(got["match"]) == match and list(got["n_admitted"]) == nadm and list(got["rbest"]) == rbest
        for i, c in enumerate(fwd):
            for s in range(2):
                if s < len(c):
                    assert got["idx"][i, s] == c[s][1] and float(got["dist"][i, s]) == c[s][0]
                else:
                    assert got["idx"][i, s] == -1 and (got["dist"][i, s] == gm.INT_MAX if ham else np.isposinf(got["dist"][i, s]))
        if gate:
            assert nadm[5] == 0 and nadm[6] == 0 and nadm[2] == 1 and list(got["idx"][2]) == [3, -1]
            assert not got["admitted"][:, 8].any()
            if not cross:                                               # a single admitted neighbour passes the ratio test
                assert got["match"][2] == 3


@pytest.mark.parametrize("integer,dim,n1,n2", [(True, 128, 40, 70), (False, 6, 40, 70), (False, 128, 30, 65), (True, 6, 9, 1)])
def test_no_gate_no_rule_is_the_matcher_oracle(integer, dim, n1, n2):
    import match_oracle as mo
    d1, d2 = gc.l2_sets(n1, n2, dim, 11, integer)
    d2[7 % n2] = d2[0]
    got = gm.match_guided(d1, d2)
    idx, dist = mo.knn2(d1, d2)
    assert np.array_equal(got["idx"], idx) and np.array_equal(got["dist"], dist)
    assert np.array_equal(got["match"], idx[:, 0]) and (got["n_admitted"] == n2).all() and (got["rbest"] == -1).all()


@pytest.mark.parametrize("name", ["general", "forward", "noisy"])
def test_epipolar_predicate_is_the_consensus_test(name):
    s = fm.with_outliers(name, 60, 0.3, 5) if name != "noisy" else fm.scene(name, 60)
    F = fm.ground_truth(s)
    p1, p2 = s["p1"].copy(), s["p2"].copy()
    p1[3] = np.nan; p2[9, 1] = np.inf
    n = len(p1)
    for t in (0.5, 3.0, 40.0):
        adm = gm.epi_admitted(F, p1, p2, t)
        a = np.repeat(p1, n, axis=0); b = np.tile(p2, (n, 1))
        with np.errstate(all="ignore"):
            want = (fm.err(F, a, b) <= t * t).reshape(n, n)
        assert np.array_equal(adm, want) and np.array_equal(adm, fm.consensus(F, a, b, t).reshape(n, n))
        assert np.array_equal(gm.epi_admitted(F.T, p2, p1, t), adm.T)              # the reverse pass: F^T with the sets swapped
        print(name, t, "admitted share %.3f, on the diagonal %d of %d" % (adm.mean(), np.diag(adm).sum(), n))
    e1, e2 = gm.epi_parts(F, p1, p2)
    f1, f2 = fm.err_parts(F, np.repeat(p1, n, axis=0), np.tile(p2, (n, 1)))
    assert np.array_equal(e1.ravel(), f1, equal_nan=True) and np.array_equal(e2.ravel(), f2, equal_nan=True)


def check_property_a(plain, guided, admitted):
    """every plain accepted match whose pair the gate admits is a guided match -> (plain accepted, of them admitted, of them kept)"""
    q = np.nonzero(plain["match"] >= 0)[0]
    adm = [i for i in q if admitted[i, plain["match"][i]]]
    kept = [i for i in adm if guided["match"][i] == plain["match"][i]]
    return len(q), len(adm), len(kept)


def mutual_pairs(plain):
    """(i, j) with j nearest to i and i nearest to j in the plain search (plain run with cross_check and ratio 1)"""
    return [(i, int(j)) for i, j in enumerate(plain["match"]) if j >= 0]


@pytest.mark.parametrize("ham", [True, False])
@pytest.mark.parametrize("gate,share", [(1, 0.05), (1, 0.5), (2, 0.05), (2, 0.5), (3, 0.05), (3, 0.5)])
def test_provable_properties_on_the_model(ham, gate, share):
    n1, n2 = 60, 80
    d1, d2 = gc.hamming_sets(n1, n2, 8, 21) if ham else gc.l2_sets(n1, n2, 16, 21, integer=True)
    d2[40:50] = d2[0:10]                                                # repeated texture: the plain ratio test rejects what a gate can recover
    p1, p2 = gc.positions(n1, n2, 21)
    F = gc.F_FORWARD if gate == 3 else gc.F_GENERAL
    p2 = gc.true_positions(gate, F, p1, p2, 30)                         # the true matches agree with the geometry
    kw = gc.gate_kwargs(gate, share, p1, p2, F=F)
    for ratio in (0.8, 1.0):
        plain = gm.match_guided(d1, d2, ratio=ratio)
        guided = gm.match_guided(d1, d2, ratio=ratio, **kw)
        a = check_property_a(plain, guided, guided["admitted"])
        print("gate", gate, "share %.3f" % guided["admitted"].mean(), "ratio", ratio, "(a) plain accepted, admitted, kept:", a,
              "guided accepted", int((guided["match"] >= 0).sum()))
        assert a[1] == a[2]
    plain = gm.match_guided(d1, d2, cross_check=True)
    guided = gm.match_guided(d1, d2, cross_check=True, **kw)
    pairs = [(i, j) for i, j in mutual_pairs(plain) if guided["admitted"][i, j]]
    print("(b) mutual pairs of the plain search %d, admitted %d" % (len(mutual_pairs(plain)), len(pairs)))
    assert all(guided["match"][i] == j for i, j in pairs)


def test_counts_cut_both_sets():
    d1, d2 = gc.hamming_sets(9, 12, 4, 2)
    p1, p2 = gc.positions(9, 12, 2)
    kw = gc.gate_kwargs(1, 0.5, p1, p2)
    full = gm.match_guided(d1[:5], d2[:7], cross_check=True, **dict(kw, pts1=p1[:5], pts2=p2[:7]))
    cut = gm.match_guided(d1, d2, cross_check=True, count1=5, count2=7, **kw)
    for k in ("match", "idx", "dist", "n_admitted"):
        assert np.array_equal(cut[k][:5], full[k])
    assert np.array_equal(cut["rbest"][:7], full["rbest"]) and (cut["rbest"][7:] == -1).all()
    assert (cut["match"][5:] == -1).all() and (cut["idx"][5:] == -1).all() and (cut["n_admitted"][5:] == 0).all()
    zero = gm.match_guided(d1, d2, cross_check=True, count1=9, count2=0, **kw)
    assert (zero["match"] == -1).all() and (zero["rbest"] == -1).all() and (zero["n_admitted"] == 0).all()
