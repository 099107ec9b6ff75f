"""gmatch_model.py -- the definition of guided descriptor matching (include/vo_mi355x.h, section "guided descriptor matching"; kernels in
csrc/vo_match.hip), restated in numpy.  OpenCV has no guided matcher, so this model is what the kernels are compared with, for equality.

One sequence at a time.  Every float64 expression below is a single IEEE operation per step in the order the kernels use (the library is built
with -ffp-contract=off), so results are equal bit for bit, not within a tolerance."""
import numpy as np

INT_MAX = np.int32(0x7fffffff)


def _w(p):
    """float32 positions, widened"""
    return np.asarray(p, np.float32).astype(np.float64).reshape(-1, 2)


def window_admitted(centers, pts2, radius):
    """(n1, n2) bool: (dx dx + dy dy) <= radius radius, dx = pts2[j].x - c[i].x in float64; any NaN -> False"""
    c, t = _w(centers), _w(pts2)
    with np.errstate(all="ignore"):
        dx = t[None, :, 0] - c[:, None, 0]; dy = t[None, :, 1] - c[:, None, 1]
        return (dx * dx + dy * dy) <= np.float64(radius) * np.float64(radius)


def epi_parts(F, pts1, pts2):
    """(e1, e2), each (n1, n2): the squared distances of pts1[i] and pts2[j] to their epipolar lines under F (x2^T F x1 = 0), the float64
    expressions of the consensus test of the fundamental-matrix search"""
    F = np.asarray(F, np.float64).reshape(9)
    p, t = _w(pts1), _w(pts2)
    x, y, u, v = p[:, None, 0], p[:, None, 1], t[None, :, 0], t[None, :, 1]
    with np.errstate(all="ignore"):
        a2, b2, c2 = (F[0] * x + F[1] * y) + F[2], (F[3] * x + F[4] * y) + F[5], (F[6] * x + F[7] * y) + F[8]
        s2, d2 = 1.0 / (a2 * a2 + b2 * b2), (u * a2 + v * b2) + c2
        a1, b1, c1 = (F[0] * u + F[3] * v) + F[6], (F[1] * u + F[4] * v) + F[7], (F[2] * u + F[5] * v) + F[8]
        s1, d1 = 1.0 / (a1 * a1 + b1 * b1), (x * a1 + y * b1) + c1
        e1, e2 = (d1 * d1) * s1, (d2 * d2) * s2
        return np.broadcast_to(e1, (len(p), len(t))), np.broadcast_to(e2, (len(p), len(t)))


def epi_admitted(F, pts1, pts2, epi_dist):
    """(n1, n2) bool: both squared distances <= epi_dist epi_dist; NaN and inf are never admitted"""
    e1, e2 = epi_parts(F, pts1, pts2)
    thr2 = np.float64(epi_dist) * np.float64(epi_dist)
    with np.errstate(invalid="ignore"):
        return (e1 <= thr2) & (e2 <= thr2)


def admitted(n1, n2, pts1=None, pts2=None, F=None, centers=None, radius=None, epi_dist=None):
    """(n1, n2) bool, the pair predicate; radius / epi_dist not None set the window / the epipolar gate"""
    adm = np.ones((n1, n2), bool)
    if radius is not None:
        adm &= window_admitted(pts1 if centers is None else centers, pts2, radius)
    if epi_dist is not None:
        adm &= epi_admitted(F, pts1, pts2, epi_dist)
    return adm


def hamming_distances(desc1, desc2):
    """(n1, n2) int32 popcounts of the xor"""
    a, b = np.asarray(desc1, np.uint8), np.asarray(desc2, np.uint8)
    return np.unpackbits(a[:, None, :] ^ b[None, :, :], axis=2).sum(2).astype(np.int32)


def l2_distances(desc1, desc2):
    """(n1, n2) float32: sqrtf((float)acc), acc the float64 sum of the squared float32 differences, accumulated in ascending k"""
    a, b = np.asarray(desc1, np.float32).astype(np.float64), np.asarray(desc2, np.float32).astype(np.float64)
    acc = np.zeros((len(a), len(b)), np.float64)
    with np.errstate(all="ignore"):
        for k in range(a.shape[1]):
            e = a[:, None, k] - b[None, :, k]
            acc = acc + e * e
        return np.sqrt(acc.astype(np.float32))


def nearest2(D, adm):
    """per row of D the two smallest admitted entries by (distance, column); NaN never enters -> idx (n, 2) int32 (-1 = none), dist (n, 2) of
    D's dtype (INT32_MAX / +inf = none), n_admitted (n,) int32"""
    n = D.shape[0]
    empty = INT_MAX if D.dtype == np.int32 else np.float32(np.inf)
    idx = np.full((n, 2), -1, np.int32); dist = np.full((n, 2), empty, D.dtype)
    for i in range(n):
        cols = [j for j in np.nonzero(adm[i])[0] if not (D.dtype != np.int32 and np.isnan(D[i, j]))]
        cols.sort(key=lambda j: (D[i, j], j))
        for s, j in enumerate(cols[:2]):
            idx[i, s] = j; dist[i, s] = D[i, j]
    return idx, dist, adm.sum(1).astype(np.int32)


def accept(idx, dist, rbest, ratio=1.0, max_dist=None, cross_check=False):
    """match (n1,) int32: idx[i][0] where every condition of the accept rule holds, else -1"""
    max_dist = np.inf if max_dist is None else float(max_dist)
    match = np.full(len(idx), -1, np.int32)
    for i in range(len(idx)):
        i0, i1 = int(idx[i, 0]), int(idx[i, 1])
        if i0 < 0:
            continue
        d0, d1 = float(dist[i, 0]), float(dist[i, 1])
        if not d0 <= max_dist:
            continue
        if not (ratio == 1.0 or i1 < 0 or d0 < float(ratio) * d1):
            continue
        if cross_check and rbest[i0] != i:
            continue
        match[i] = i0
    return match


def match_guided(desc1, desc2, pts1=None, pts2=None, F=None, centers=None, radius=None, epi_dist=None, ratio=1.0, max_dist=None,
                 cross_check=False, count1=None, count2=None):
    """one sequence of VoContext.match_guided -> dict match, idx, dist, n_admitted (n1 rows), rbest (n2 rows), admitted (the (n1, n2) predicate,
    False for rows that do not exist)"""
    ham = np.asarray(desc1).dtype == np.uint8
    n1, n2 = len(desc1), len(desc2)
    m1 = n1 if count1 is None else int(count1)
    m2 = n2 if count2 is None else int(count2)
    cut1 = lambda a: None if a is None else np.asarray(a)[:m1]      # noqa: E731
    cut2 = lambda a: None if a is None else np.asarray(a)[:m2]      # noqa: E731
    adm = admitted(m1, m2, cut1(pts1), cut2(pts2), F, cut1(centers), radius, epi_dist)
    D = (hamming_distances if ham else l2_distances)(np.asarray(desc1)[:m1], np.asarray(desc2)[:m2])
    empty = INT_MAX if ham else np.float32(np.inf)
    idx = np.full((n1, 2), -1, np.int32); dist = np.full((n1, 2), empty, D.dtype); nadm = np.zeros(n1, np.int32)
    idx[:m1], dist[:m1], nadm[:m1] = nearest2(D, adm)
    rbest = np.full(n2, -1, np.int32)
    if cross_check:
        rbest[:m2] = nearest2(np.ascontiguousarray(D.T), adm.T)[0][:, 0]
    match = accept(idx, dist, rbest, ratio, max_dist, cross_check)
    full = np.zeros((n1, n2), bool); full[:m1, :m2] = adm
    return dict(match=match, idx=idx, dist=dist, n_admitted=nadm, rbest=rbest, admitted=full)
