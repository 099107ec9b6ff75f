"""Inputs of the guided-matching tests (tests/test_gmatch_model.py on the model, tests/test_gpu_gmatch.py on the kernels): descriptor sets with
true matches and repeated rows, positions and fundamental matrices whose gates admit a chosen share of the pairs, and the edge rows.  The gate
distances are quantiles of quantities computed here with plain numpy and tests/fundamental_model.py, never with the code under test."""
import numpy as np

import fundamental_model as fm

SIZE = 100.0                                            # positions are drawn in [-SIZE / 2, SIZE / 2]^2
# pure forward motion, t = (0, 0, 1): F = [t]x.  The epipolar line of x1 is (-y1, x1, 0): through the origin, and a^2 + b^2 = 0 for x1 = (0, 0)
F_FORWARD = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
# a general two-view geometry (rotation and translation), moved to the centred pixel coordinates used here
_T = np.array([[1.0, 0.0, 620.0], [0.0, 1.0, 188.0], [0.0, 0.0, 1.0]])
F_GENERAL = fm.unit(_T.T @ fm.ground_truth(fm.scene("general")) @ _T)


def hamming_sets(n1, n2, nbytes, seed):
    """random bytes; the first min(n1, n2) // 2 train rows are queries with a few bits flipped"""
    rng = np.random.default_rng([seed, n1, n2, nbytes])
    d1 = rng.integers(0, 256, (n1, nbytes), dtype=np.uint8)
    d2 = rng.integers(0, 256, (n2, nbytes), dtype=np.uint8)
    k = min(n1, n2) // 2
    d2[:k] = d1[:k] ^ (rng.integers(0, 256, (k, nbytes), dtype=np.uint8) & rng.integers(0, 256, (k, nbytes), dtype=np.uint8)
                       & rng.integers(0, 256, (k, nbytes), dtype=np.uint8))
    return d1, d2


def l2_sets(n1, n2, dim, seed, integer):
    """integer: 0..255 valued rows (SIFT's range: every sum is exact); else random floats.  Half of the train rows are noisy copies of queries"""
    rng = np.random.default_rng([seed, n1, n2, dim, int(integer)])
    if integer:
        d1 = np.minimum(np.floor(rng.gamma(0.6, 30.0, (n1, dim))), 255).astype(np.float32)
        d2 = np.minimum(np.floor(rng.gamma(0.6, 30.0, (n2, dim))), 255).astype(np.float32)
        k = min(n1, n2) // 2
        d2[:k] = np.clip(d1[:k] + rng.integers(-2, 3, (k, dim)), 0, 255).astype(np.float32)
    else:
        d1 = rng.standard_normal((n1, dim)).astype(np.float32)
        d2 = rng.standard_normal((n2, dim)).astype(np.float32)
        k = min(n1, n2) // 2
        d2[:k] = d1[:k] + (0.05 * rng.standard_normal((k, dim))).astype(np.float32)
    return d1, d2


def positions(n1, n2, seed):
    rng = np.random.default_rng([seed, n1, n2, 17])
    return (rng.uniform(-SIZE / 2, SIZE / 2, (n1, 2)).astype(np.float32), rng.uniform(-SIZE / 2, SIZE / 2, (n2, 2)).astype(np.float32))


def _quantile(values, share):
    v = np.sort(values[np.isfinite(values)].ravel())
    return float(v[min(len(v) - 1, max(0, int(round(share * len(v))) - 1))])


def radius_for(centers, pts2, share):
    """the radius that admits about `share` of the pairs: that quantile of the centre-to-point distances"""
    c, t = np.asarray(centers, np.float64), np.asarray(pts2, np.float64)
    return max(_quantile(np.hypot(t[None, :, 0] - c[:, None, 0], t[None, :, 1] - c[:, None, 1]), share), 1e-3)


def epi_dist_for(F, pts1, pts2, share):
    """the epipolar distance that admits about `share` of the pairs: that quantile of sqrt(err) of tests/fundamental_model.py over all pairs"""
    n1, n2 = len(pts1), len(pts2)
    e = fm.err(F, np.repeat(np.asarray(pts1, np.float32), n2, axis=0), np.tile(np.asarray(pts2, np.float32), (n1, 1)))
    return max(_quantile(np.sqrt(e), share), 1e-3)


def gate_kwargs(gate, share, pts1, pts2, F=F_GENERAL, centers=None):
    """keywords of match_guided for gate 0..3 admitting about `share` of the pairs; with both gates each gets the same quantile of its own
    distance, found by bisection on the joint share"""
    kw = {}
    if gate:
        kw.update(pts1=pts1, pts2=pts2)
    c = pts1 if centers is None else centers
    each = share
    if gate == 3:
        Dw = np.hypot(*(np.asarray(pts2, np.float64)[None, :, k] - np.asarray(c, np.float64)[:, None, k] for k in (0, 1)))
        De = np.sqrt(fm.err(F, np.repeat(np.asarray(pts1, np.float32), len(pts2), axis=0),
                            np.tile(np.asarray(pts2, np.float32), (len(pts1), 1)))).reshape(Dw.shape)
        lo, hi = share, 1.0
        for _ in range(30):
            each = 0.5 * (lo + hi)
            joint = ((Dw <= _quantile(Dw, each)) & (De <= _quantile(De, each))).mean()
            lo, hi = (each, hi) if joint < share else (lo, each)
    if gate & 1:
        kw.update(radius=radius_for(c, pts2, each))
        if centers is not None:
            kw.update(centers=centers)
    if gate & 2:
        kw.update(F=F, epi_dist=epi_dist_for(F, pts1, pts2, each))
    return kw


def true_positions(gate, F, pts1, pts2, k):
    """pts2 with its first k rows moved to where the first k queries would be seen: a hundredth further from the centre (a nearby point, and on
    the query's epipolar line under F_FORWARD), or under the epipolar gate alone the foot of the query on its epipolar line under F"""
    p2 = pts2.copy()
    for i in range(k):
        p2[i] = on_epiline(F, pts1[i]) if gate == 2 else pts1[i] * np.float32(1.01)
    return p2


def plant_edges(pts1, pts2, gate, F, lone_q, lone_t, none_q, nan_q, nan_t):
    """edge rows, written into copies of the position sets (indices beyond a set are skipped):
    none_q   a query far from everything: no admitted row under either gate
    lone_q   a query far from everything but train row lone_t: under the window gate that row sits on it (with both gates F must be
             F_FORWARD, under which a point lies on its own epipolar line), under the epipolar gate alone on its epipolar line to float32 rounding
    nan_q, nan_t  a NaN coordinate"""
    p1, p2 = pts1.copy(), pts2.copy()
    if none_q < len(p1):
        p1[none_q] = (-9000.0, 7000.0)
    if lone_q < len(p1) and lone_t < len(p2):
        p1[lone_q] = (8000.0, 6000.0)
        p2[lone_t] = p1[lone_q] if gate & 1 else on_epiline(F, p1[lone_q])
    if nan_q < len(p1):
        p1[nan_q, 0] = np.nan
    if nan_t < len(p2):
        p2[nan_t, 1] = np.nan
    return p1, p2


def on_epiline(F, x1):
    """the float32 point of view 2 nearest to x1 on x1's epipolar line under F (x1 itself where the line is degenerate)"""
    a, b, c = np.asarray(F, np.float64).reshape(3, 3) @ np.array([float(x1[0]), float(x1[1]), 1.0])
    if a * a + b * b == 0:
        return np.asarray(x1, np.float32)
    k = (a * float(x1[0]) + b * float(x1[1]) + c) / (a * a + b * b)
    return np.array([float(x1[0]) - k * a, float(x1[1]) - k * b], np.float32)
