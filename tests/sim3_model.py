"""numpy model of the Sim(3) / rigid 3D-3D alignment search (csrc/vo_sim3.hip: three-point RANSAC, Umeyama re-fit), its high-precision
truth, the scenes of the tests and the bounds the library is held to.

Plain numpy, float64 and LAPACK's SVD; no GPU.  Written from Umeyama 1991 ("Least-squares estimation of transformation parameters between
two point patterns", eqs. 34-43) and Horn 1987; it shares no numerical step with the kernel (one-sided Jacobi rotations in registers,
cross products for the third singular vectors, another reduction tree):

  sample3        the documented draw of hypothesis h (the generator of the other searches, three draws)
  umeyama        centroids, Sigma = 1/m sum (y - yc)(x - xc)^T, U D V^T = Sigma by LAPACK, S = diag(1, 1, sign(det U det V)), R = U S V^T,
                 s = tr(D S) / var_x (or 1), t = yc - s R xc; computed in two passes (centroids first, central moments about them second)
  solve3         the minimal model of a sample: degenerate where, in either set, |(b - a) x (c - a)|^2 <= 1e-10 |b - a|^2 |c - a|^2, where a
                 coordinate is not finite, or (with scale) where s is not finite or <= 0
  err            |y - (s R x + t)|^2 in float64, the same expressions as the kernel, and err_band: how far it may move when the model moves
  search         the whole search restated: rounds of 256, most inliers, ties to the smallest h, at least 3, RANSACUpdateNumIters with 3 model
                 points -- and `decided`: whether a solver whose every model lies within SOLVE_FACTOR x 2^-52 x kappa of this model's must
                 return the same winner, count, mask, number of hypotheses and number of degenerate samples
  fit / finish   Umeyama over a consensus set; the set is degenerate where the second eigenvalue of either set's scatter matrix
                 sum (x - xc)(x - xc)^T is <= 1e-10 of the first (the squared singular values of the centred set)
  truth          the same closed form in 40 digits (mpmath; numpy's longdouble where mpmath is missing) with its own Jacobi SVD

kappa = s1 / (s2 + d3) with s1 >= s2 the two largest singular values of Sigma and d3 = sign(det U det V) s3 the signed third: the rotation
about the axis the two weakest directions span is fixed by s2 + d3 alone (Umeyama's lemma; a three-point Sigma has d3 = 0, a mirrored cloud
d3 < 0), so its sensitivity to rounding grows as that sum falls against s1.  A model is the 13 numbers (s, R row-major, t); two models are
compared by diff(): the largest of |dR| (entries), |ds| / s and |dt| / (|yc| + s (|xc| + sigma_x)).

Every bound has the form FACTOR x 2^-52 x kappa.  FACTOR is 4 x the worst ratio of this float64 model to the 40-digit truth (measured: 3.00
for a three-point sample, 7.93 for a set; SOLVE_FACTOR = 13, REFIT_FACTOR = 32), measured by
tests/test_sim3_model.py over the scene families named there and never on the kernel: a kernel that rotates instead of calling LAPACK and
sums in another order is equally valid but may lose a few more bits.
"""
import math

import numpy as np

EPS = 2.0 ** -52
BATCH = 256
THRESHOLD, CONFIDENCE, MAX_ITERS = 3.0, 0.99, 1000
DEGENERATE = 1e-10                # sample: squared sine of the triangle; set: second eigenvalue of the scatter matrix over the first
# A degeneracy figure within this factor of DEGENERATE may be judged otherwise by a correct solver.  What rounding can do is far less: the
# cross product of two nearly parallel float64 edges at sine 1e-5 is good to 2^-52 / 1e-5 = 2e-11 relative, and the second eigenvalue of a
# scatter matrix to a few 2^-52 of the first, 1e-5 of itself at the ratio 1e-10.  A factor of two leaves room for any order of evaluation
AMBIGUOUS = 2.0
KAPPA_CUT = 1e8                   # a winner over this kappa is not compared (the search is then not `decided`)
_M64 = (1 << 64) - 1

# ---- measured constants ---------------------------------------------------------------------------------------------------------------
# tests/test_sim3_model.py measures each ratio again on the model alone, prints it, and asserts that each factor is 4 x the recorded ratio
# (rounded up) and that the fresh measurement does not exceed the record.
# diff(solve3(sample), truth) <= SOLVE_FACTOR x 2^-52 x kappa over the minimal samples of every family
SOLVE_FACTOR = 13.0
# diff(fit(set), truth) <= REFIT_FACTOR x 2^-52 x kappa over the consensus sets of every family
REFIT_FACTOR = 32.0
MEASURED = dict(solve=3.01, refit=7.94)


# =========================================================================================================================================
# the sample generator and the iteration bound
# =========================================================================================================================================
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def sample3(seed, h, n):
    """three distinct indices in [0, n) of hypothesis h: draw k is splitmix64(seed, h, k) mod n, repeats are skipped"""
    idx, k = [], 0
    while len(idx) < 3:
        r = splitmix64(((seed & 0xFFFFFF) << 40) ^ ((h & 0xFFFFFFFF) << 8) ^ (k & 0xFF)) if k < 256 else splitmix64(k)
        i = int((r >> 11) % n)
        k += 1
        if i not in idx:
            idx.append(i)
    return idx


def ransac_num_iters(conf, outlier_ratio, max_iters=MAX_ITERS, model_points=3):
    """OpenCV's RANSACUpdateNumIters: log(1 - p) / log(1 - (1 - ep)^m), rounded to nearest-even, capped"""
    tiny = np.finfo(float).tiny
    p, ep = min(max(conf, 0.0), 1.0), min(max(outlier_ratio, 0.0), 1.0)
    num = max(1.0 - p, tiny)
    den = 1.0 - (1.0 - ep) ** model_points
    if den < tiny:
        return 0
    num, den = math.log(num), math.log(den)
    if den >= 0 or -num >= max_iters * (-den):
        return max_iters
    return int(round(num / den))


def widen(p):
    """float32 points widened to float64 (exact)"""
    return np.asarray(p, np.float32).astype(np.float64).reshape(-1, 3)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# =========================================================================================================================================
# Umeyama's closed form
# =========================================================================================================================================
def pack(s, R, t):
    return np.concatenate([[s], np.asarray(R, float).reshape(9), np.asarray(t, float).reshape(3)])


def unpack(m):
    m = np.asarray(m, float).reshape(13)
    return float(m[0]), m[1:10].reshape(3, 3), m[10:13]


def similarity(m):
    """the 4 x 4 matrix S of a model: (y, 1) = S (x, 1)"""
    s, R, t = unpack(m)
    S = np.eye(4)
    S[:3, :3], S[:3, 3] = s * R, t
    return S


def moments(X, Y):
    """two passes over float64 rows: -> (xc, yc, Sigma = 1/m sum (y - yc)(x - xc)^T, Cxx = sum (x - xc)(x - xc)^T, Cyy)"""
    m = len(X)
    xc, yc = X.sum(0) / m, Y.sum(0) / m
    A, B = X - xc, Y - yc
    return xc, yc, (B.T @ A) / m, A.T @ A, B.T @ B


def umeyama(X, Y, with_scale=True):
    """X, Y (m, 3) float64 -> dict m (13), s, R, t, kappa, sv = (s1, s2, d3), tscale; None if an entry is not finite or (with scale) s <= 0"""
    with np.errstate(all="ignore"):
        xc, yc, Sg, Cxx, _ = moments(X, Y)
        if not np.all(np.isfinite(Sg)):
            return None
        U, D, Vt = np.linalg.svd(Sg)
        sg = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0 else -1.0
        S = np.diag([1.0, 1.0, sg])
        R = U @ S @ Vt
        varx = np.trace(Cxx) / len(X)
        s = float((D[0] + D[1]) + sg * D[2]) / varx if with_scale else 1.0
        t = yc - s * (R @ xc)
        mdl = pack(s, R, t)
        if not np.all(np.isfinite(mdl)) or not s > 0:
            return None
        return dict(m=mdl, s=s, R=R, t=t, kappa=float(D[0] / (D[1] + sg * D[2])) if D[1] + sg * D[2] > 0 else math.inf,
                    sv=(float(D[0]), float(D[1]), float(sg * D[2])), tscale=float(np.linalg.norm(yc) + s * (np.linalg.norm(xc) + math.sqrt(varx))))


def diff(got, ref, tscale):
    """two models (13) -> max of |dR|, |ds| / s, |dt| / tscale"""
    s1, R1, t1 = unpack(got)
    s0, R0, t0 = unpack(ref)
    return float(max(np.abs(R1 - R0).max(), abs(s1 - s0) / s0, np.abs(t1 - t0).max() / tscale))


def sine2(a, b, c):
    """|(b - a) x (c - a)|^2 / (|b - a|^2 |c - a|^2): 0 for coincident points"""
    u, v = b - a, c - a
    w = np.cross(u, v)
    den = (u @ u) * (v @ v)
    return float((w @ w) / den) if den > 0 else 0.0


def solve3(x, y, with_scale=True):
    """the minimal model of three pairs (float64 rows) -> dict of umeyama + ambiguous, or dict m=None, ambiguous"""
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))):
        return dict(m=None, ambiguous=False)
    sx, sy = sine2(*x), sine2(*y)
    amb = any(DEGENERATE / AMBIGUOUS < v < DEGENERATE * AMBIGUOUS for v in (sx, sy))
    if sx <= DEGENERATE or sy <= DEGENERATE:
        return dict(m=None, ambiguous=amb)
    u = umeyama(x, y, with_scale)
    if u is None:
        return dict(m=None, ambiguous=True)
    u["ambiguous"] = amb
    return u


# =========================================================================================================================================
# the consensus test
# =========================================================================================================================================
def err(m, src, dst):
    """|y - (s R x + t)|^2 per pair, the kernel's expressions; inf where it is not finite (never an inlier)"""
    m = np.asarray(m, float)
    X, Y = widen(src), widen(dst)
    with np.errstate(all="ignore"):
        d = [Y[:, k] - (m[0] * ((m[1 + 3 * k] * X[:, 0] + m[2 + 3 * k] * X[:, 1]) + m[3 + 3 * k] * X[:, 2]) + m[10 + k]) for k in range(3)]
        e = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    e[~np.isfinite(e)] = np.inf
    return e


def err_band(m, src, dst, delta, tscale):
    """how far err may move at each pair when the model moves by delta in the sense of diff(): an entry of R by delta, s by delta s, t by
    delta tscale -- a component of y - (s R x + t) then moves by at most D = delta (2 s |x|_1 + tscale) (and by the roundings of its own
    evaluation, at most 8 x 2^-52 (|y| + s |x|_1 + |t|), covered by adding that to D), and err by 2 |d|_1 D + 3 D^2"""
    s, R, t = unpack(m)
    X, Y = widen(src), widen(dst)
    with np.errstate(all="ignore"):
        x1 = np.abs(X).sum(1)
        D = delta * (2 * s * x1 + tscale) + 8 * EPS * (np.abs(Y).max(1) + s * x1 + np.abs(t).max())
        d1 = np.abs(Y - (s * (X @ R.T) + t)).sum(1)
        b = 2 * d1 * D + 3 * D * D
    b[~np.isfinite(b)] = np.inf
    b[~(np.all(np.isfinite(X), 1) & np.all(np.isfinite(Y), 1))] = 0.0      # err is inf there for every solver
    return b


def consensus(m, src, dst, thr=THRESHOLD):
    return err(m, src, dst) <= thr * thr


# =========================================================================================================================================
# the search
# =========================================================================================================================================
def hypothesis(src, dst, seed, h, thr=THRESHOLD, with_scale=True):
    """-> (idx, dict of solve3, dict cnt, lo, hi or None): lo / hi bound the count of a solver whose model lies within
    SOLVE_FACTOR x 2^-52 x kappa of this one"""
    n = len(src)
    idx = sample3(seed, h, n)
    u = solve3(widen(src)[idx], widen(dst)[idx], with_scale)
    if u["m"] is None:
        return idx, u, None
    e = err(u["m"], src, dst)
    band = err_band(u["m"], src, dst, SOLVE_FACTOR * EPS * u["kappa"], u["tscale"])
    lo, hi = int((e + band <= thr * thr).sum()), int((e - band <= thr * thr).sum())
    return idx, u, dict(cnt=int((e <= thr * thr).sum()), lo=lo, hi=hi)


def search(src, dst, thr=THRESHOLD, conf=CONFIDENCE, max_iters=MAX_ITERS, seed=0, with_scale=True):
    """the whole search -> dict best (-1: none), hypotheses, m0, mask, count, degenerate, kappa, tscale (of the winner), decided, why"""
    n = len(src)
    niters, h_done, best, best_count, m0, kappa, tscale, degenerate = max_iters, 0, -1, 2, None, math.inf, 1.0, 0
    decided, why, seen = True, [], []
    max_lo = max_hi = 2
    max_rounds = -(-max_iters // BATCH)
    for _ in range(max_rounds):
        for h in range(h_done, h_done + BATCH):
            _, u, row = hypothesis(src, dst, seed, h, thr, with_scale)
            if u["ambiguous"]:
                decided = False
                why.append("sample %d is within %g of a tolerance" % (h, AMBIGUOUS))
            if row is None:
                degenerate += 1
                continue
            max_lo, max_hi = max(max_lo, row["lo"]), max(max_hi, row["hi"])
            seen.append((h, row))
            if row["cnt"] > best_count:
                best, best_count, m0, kappa, tscale = h, row["cnt"], u["m"], u["kappa"], u["tscale"]
        h_done += BATCH
        if max_lo != max_hi:                                    # the running best's count decides the bound of this round
            decided = False
            why.append("after %d hypotheses the best count lies in %d .. %d" % (h_done, max_lo, max_hi))
        if best >= 0:
            niters = min(niters, ransac_num_iters(conf, (n - best_count) / n, max_iters))
        if h_done >= niters:
            break
    if best >= 0:
        for h, row in seen:
            if h == best:
                if row["lo"] != row["hi"]:
                    decided = False
                    why.append("the winner's count lies in %d .. %d" % (row["lo"], row["hi"]))
            elif row["hi"] > best_count or (h < best and row["hi"] == best_count):
                decided = False
                why.append("hypothesis %d may reach %d" % (h, row["hi"]))
        if not kappa <= KAPPA_CUT:
            decided = False
            why.append("the winner's kappa is %.3g" % kappa)
    mask = consensus(m0, src, dst, thr) if best >= 0 else np.zeros(n, bool)
    return dict(best=best, hypotheses=h_done, m0=m0, mask=mask, count=best_count if best >= 0 else 0, degenerate=degenerate, kappa=kappa,
                tscale=tscale, decided=decided, why=why)


# =========================================================================================================================================
# the fit over a set
# =========================================================================================================================================
def set_ratios(X, Y):
    """second eigenvalue of each set's scatter matrix over the first -> (rx, ry); nan for an empty or one-point set"""
    with np.errstate(all="ignore"):
        _, _, _, Cxx, Cyy = moments(X, Y)
        out = []
        for C in (Cxx, Cyy):
            if not np.all(np.isfinite(C)):
                out.append(math.nan)
                continue
            lam = np.linalg.eigvalsh(C)
            out.append(float(lam[1] / lam[2]) if lam[2] > 0 else math.nan)
    return tuple(out)


def fit(src, dst, mask=None, with_scale=True):
    """Umeyama over the pairs of `mask` (None: all) with finite coordinates -> dict of umeyama + mask, count, ratios, ambiguous; m=None with
    fewer than 3 pairs, a degenerate set or a fit that is not finite"""
    X, Y = widen(src), widen(dst)
    keep = np.all(np.isfinite(X), 1) & np.all(np.isfinite(Y), 1)
    if mask is not None:
        keep &= np.asarray(mask, bool)
    out = dict(m=None, mask=keep, count=int(keep.sum()), ratios=(math.nan, math.nan), ambiguous=False)
    if out["count"] < 3:
        return out
    out["ratios"] = set_ratios(X[keep], Y[keep])
    out["ambiguous"] = any(DEGENERATE / AMBIGUOUS < v < DEGENERATE * AMBIGUOUS for v in out["ratios"])
    if not all(v > DEGENERATE for v in out["ratios"]):
        return out
    u = umeyama(X[keep], Y[keep], with_scale)
    if u is not None:
        out.update(u)
    return out


def cost(m, src, dst, mask):
    """sum of squared errors over `mask` under the model m"""
    return float(err(m, src, dst)[np.asarray(mask, bool)].sum())


def finish(src, dst, found, refit=1, with_scale=True):
    """what the search returns for the result `found` of search(): dict m, refit (which of the two), cost, fit (the dict of fit() or None)"""
    if found["best"] < 0:
        return dict(m=None, refit=0, cost=math.nan, fit=None)
    f = fit(src, dst, found["mask"], with_scale) if refit else None
    if f is not None and f["m"] is not None:
        return dict(m=f["m"], refit=1, cost=cost(f["m"], src, dst, found["mask"]), fit=f)
    return dict(m=found["m0"], refit=0, cost=cost(found["m0"], src, dst, found["mask"]), fit=f)


# =========================================================================================================================================
# the truth: the same closed form in 40 digits, with its own (one-sided Jacobi) SVD
# =========================================================================================================================================
try:
    import mpmath as _mp
    _mp.mp.dps = 40
    HP, HP_NAME, _sqrt = _mp.mpf, "mpmath at 40 digits", _mp.sqrt
except ImportError:                                             # pragma: no cover
    HP, HP_NAME, _sqrt = np.longdouble, "numpy longdouble", np.sqrt


def _hp(x):
    return HP(float(x))


def truth(X, Y, with_scale=True):
    """X, Y (m, 3) float64 -> the model (13) of Umeyama's closed form in high precision, rounded to float64"""
    m = len(X)
    Xh, Yh = [[_hp(v) for v in r] for r in X], [[_hp(v) for v in r] for r in Y]
    xc = [sum(r[k] for r in Xh) / m for k in range(3)]
    yc = [sum(r[k] for r in Yh) / m for k in range(3)]
    A = [[sum((Yh[i][j] - yc[j]) * (Xh[i][k] - xc[k]) for i in range(m)) / m for k in range(3)] for j in range(3)]
    varx = sum((Xh[i][k] - xc[k]) ** 2 for i in range(m) for k in range(3)) / m
    Sg = [row[:] for row in A]
    V = [[HP(1) if i == j else HP(0) for j in range(3)] for i in range(3)]
    tol = HP(10) ** -70 if HP is not np.longdouble else HP(2.0) ** -126
    for _ in range(200):
        changed = False
        for p in range(2):
            for q in range(p + 1, 3):
                al = sum(A[k][p] * A[k][p] for k in range(3)); be = sum(A[k][q] * A[k][q] for k in range(3))
                ga = sum(A[k][p] * A[k][q] for k in range(3))
                if ga * ga > tol * (al * be):
                    changed = True
                    zeta = (be - al) / (2 * ga)
                    tt = (1 if zeta >= 0 else -1) / (abs(zeta) + _sqrt(1 + zeta * zeta))
                    cs = 1 / _sqrt(1 + tt * tt); sn = cs * tt
                    for k in range(3):
                        A[k][p], A[k][q] = cs * A[k][p] - sn * A[k][q], sn * A[k][p] + cs * A[k][q]
                        V[k][p], V[k][q] = cs * V[k][p] - sn * V[k][q], sn * V[k][p] + cs * V[k][q]
        if not changed:
            break
    nn = [sum(A[k][j] * A[k][j] for k in range(3)) for j in range(3)]
    o = sorted(range(3), key=lambda j: -nn[j])
    s1, s2 = _sqrt(nn[o[0]]), _sqrt(nn[o[1]])
    u1, u2 = [A[k][o[0]] / s1 for k in range(3)], [A[k][o[1]] / s2 for k in range(3)]
    v1, v2 = [V[k][o[0]] for k in range(3)], [V[k][o[1]] for k in range(3)]
    cr = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    u3, v3 = cr(u1, u2), cr(v1, v2)
    d3 = sum(u3[i] * sum(Sg[i][k] * v3[k] for k in range(3)) for i in range(3))
    R = [[u1[i] * v1[j] + u2[i] * v2[j] + u3[i] * v3[j] for j in range(3)] for i in range(3)]
    s = (s1 + s2 + d3) / varx if with_scale else HP(1)
    t = [yc[i] - s * sum(R[i][k] * xc[k] for k in range(3)) for i in range(3)]
    return np.array([float(s)] + [float(R[i][j]) for i in range(3) for j in range(3)] + [float(v) for v in t])


# =========================================================================================================================================
# scenes
# =========================================================================================================================================
def rotation(rng):
    """a uniformly drawn proper rotation"""
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


FAMILIES = ("general", "planar", "near_collinear", "two_equal", "mirrored", "small_scale", "large_scale", "far_centroid")


def family(name, n, seed):
    """a cloud of one of the scene families with its transformed copy -> dict src, dst (n, 3) float32, s, R, t (the true transform)"""
    rng = np.random.default_rng([seed, FAMILIES.index(name)])
    X = rng.uniform(-10, 10, (n, 3))
    s, R, t = 1.3, rotation(rng), rng.uniform(-5, 5, 3)
    if name == "planar":
        X[:, 2] = 0.0
        X = X @ rotation(rng).T
    elif name == "near_collinear":
        X[:, 1:] *= 1e-3
        X = X @ rotation(rng).T
    elif name == "two_equal":
        X = rng.normal(size=(n, 3)) * np.array([8.0, 3.0, 3.0 * (1 + 1e-6)])
    elif name == "small_scale":
        s = 1e-3
    elif name == "large_scale":
        s = 1e3
    elif name == "far_centroid":
        X += np.array([1e5, -2e5, 1.5e5])                       # 1e4 x the spread
    src = X.astype(np.float32)
    Y = s * (src.astype(np.float64) @ R.T) + t
    if name == "mirrored":
        Y = Y * np.array([1.0, 1.0, -1.0])
    Y = Y + rng.normal(0, 1e-3 * s, Y.shape)
    return dict(name=name, src=src, dst=Y.astype(np.float32), s=s, R=R, t=t)


def cloud(n, n_in, seed, s=1.3, noise=1e-3, planar=False, mirror=False, box=10.0):
    """n pairs of which the first n_in (shuffled afterwards) obey dst = s R src + t + noise and the rest are gross outliers: dst drawn
    anew in a box of 4 x the cloud's -> dict src, dst float32, s, R, t, inliers (bool)"""
    rng = np.random.default_rng([seed, 4242])
    X = rng.uniform(-box, box, (n, 3))
    if planar:
        X[:, 2] = 0.0
        X = X @ rotation(rng).T
    R, t = rotation(rng), rng.uniform(-5, 5, 3)
    src = X.astype(np.float32)
    Y = s * (src.astype(np.float64) @ R.T) + t
    if mirror:
        Y = Y * np.array([1.0, 1.0, -1.0])
    Y = Y + rng.normal(0, noise, Y.shape)
    inl = np.zeros(n, bool)
    inl[:n_in] = True
    Y[~inl] = rng.uniform(-4 * box * s, 4 * box * s, (n - n_in, 3))
    o = rng.permutation(n)
    return dict(src=src[o], dst=Y[o].astype(np.float32), s=s, R=R, t=t, inliers=inl[o])


def collinear_consensus():
    """27 pairs, dst = 2 Rz(90 deg) src + (1, -2, 3) exactly in float32: 24 on the line y = z = 0 (four within 2^-7 of the origin, twenty
    from x = 2.5 to 3.1), one point d = 2^-16 off it at the origin, two gross outliers.  A sample is a triangle only with the off-line point
    and a near one: its sine^2 is at least d^2 / (4 x 2^-14) = 1e-6, and its model holds all 25.  With a far point at the first vertex the
    sine^2 is d^2 / 2.5^2 = 3.7e-11 or less, and the scatter matrix of the 25 has a second eigenvalue of about d^2 / 32 = 7e-12 of the
    first: the set is degenerate although the winning sample is not"""
    d = 2.0 ** -16
    xs = [2.0 ** -8, -2.0 ** -8, 2.0 ** -7, -2.0 ** -7] + [2.5 + i / 32.0 for i in range(20)]
    src = np.array([[0.0, d, 0.0]] + [[x, 0.0, 0.0] for x in xs] + [[3.0, 40.0, -20.0], [-30.0, 5.0, 60.0]], np.float32)
    X = src.astype(np.float64)
    Y = 2.0 * np.stack([-X[:, 1], X[:, 0], X[:, 2]], 1) + np.array([1.0, -2.0, 3.0])
    Y[25:] += np.array([[50.0, -70.0, 90.0], [-80.0, 60.0, 40.0]])
    dst = Y.astype(np.float32)
    assert np.array_equal(dst.astype(np.float64)[:25], Y[:25])
    return dict(src=src, dst=dst, s=2.0, inliers=np.arange(27) < 25)


# ---- the problems of the GPU tests -------------------------------------------------------------------------------------------------------
# Each entry: name -> (scene function, search keywords).  tests/test_sim3_model.py asserts for every one that the model's own search is
# `decided`; where the first seed does not give that, the first one that does is recorded here.
THR = 0.1                         # the threshold of the GPU scenes, in dst's units: 100 x the noise, 1 / 1000 of the outliers' box
SEARCH_SEED = 7
COLLINEAR_SEED = 30               # of collinear_consensus: the first from 7 up whose winner is a triangle of the off-line and two near points
STRIDE_NS = (63, 64, 65, 257, 300)


def stride_scene(n):
    return cloud(n, int(round(0.7 * n)), seed=100 + n)


def rounds_scene():
    """n = 200 with 40 inliers and next to no noise: every all-inlier sample holds the 40, the bound is 573 and the search takes three rounds"""
    return cloud(200, 40, seed=31, noise=1e-5)


def batch_scenes():
    """three problems of n = 120 whose searches stop after one, two and three rounds"""
    return [cloud(120, k, seed=50 + i, s=sc, noise=1e-5) for i, (k, sc) in enumerate(((110, 0.5), (28, 1.0), (24, 3.0)))]


def nan_scene():
    """stride_scene(65) with three rows made NaN: one coordinate of src, one of dst, a whole row"""
    s = dict(stride_scene(65))
    src, dst = s["src"].copy(), s["dst"].copy()
    src[5, 1] = np.nan; dst[17, 2] = np.nan; src[40] = np.nan
    inl = s["inliers"].copy()
    inl[[5, 17, 40]] = False
    s.update(src=src, dst=dst, inliers=inl)
    return s


def landmark_scene():
    """two maps of 100 landmarks: map 2 = 0.4 R map 1 + t with 1 mm noise, its list shuffled; one match per landmark of map 1, 30 of them
    to a wrong landmark of map 2 -> dict p1, p2 (100, 3) float64, pairs (100, 2) int (index into map 1, into map 2), good (bool), src, dst
    (the float32 pairs as Extractor.align_landmarks forms them), s, R, t"""
    rng = np.random.default_rng([77, 1])
    n = 100
    p1 = rng.uniform(-10, 10, (n, 3))
    s, R, t = 0.4, rotation(rng), rng.uniform(-5, 5, 3)
    perm = rng.permutation(n)
    p2 = np.zeros((n, 3))
    p2[perm] = s * (p1 @ R.T) + t + rng.normal(0, 1e-3, (n, 3))
    train = perm.copy()
    bad = np.sort(rng.choice(n, 30, replace=False))
    for i in bad:
        train[i] = (perm[i] + 1 + rng.integers(0, n - 1)) % n
    good = np.ones(n, bool)
    good[bad] = False
    pairs = np.stack([np.arange(n), train], 1)
    return dict(p1=p1, p2=p2, pairs=pairs, good=good, inliers=good, src=p1[pairs[:, 0]].astype(np.float32), dst=p2[pairs[:, 1]].astype(np.float32),
                s=s, R=R, t=t)


def _pose(Rc, c):
    H = np.eye(4)
    H[:3, :3], H[:3, 3] = Rc, -Rc @ c
    return H


def trajectory_scene(outliers=0, s=2.5):
    """40 world->camera poses of an estimated trajectory (a curved path 20 long) and its ground truth: centres s R0 c + t0 with 1 cm noise;
    `outliers`: that many estimated poses moved 50 away -> dict est, gt (40, 4, 4), centres_est, centres_gt (40, 3), good (bool), src, dst
    (float32 centres), s, R, t"""
    rng = np.random.default_rng([78, 2])
    m = 40
    k = np.arange(m, dtype=float)
    c = np.stack([0.5 * k, 3.0 * np.sin(0.2 * k), 0.005 * k * k], 1)
    R0, t0 = rotation(rng), rng.uniform(-20, 20, 3)
    cg = s * (c @ R0.T) + t0 + rng.normal(0, 0.01, (m, 3))
    good = np.ones(m, bool)
    if outliers:
        bad = np.sort(rng.choice(m, outliers, replace=False))
        good[bad] = False
        d = rng.normal(size=(outliers, 3))
        c[bad] += 50.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    est, gt = [], []
    for i in range(m):
        Rc = rotation(rng)
        est.append(_pose(Rc, c[i]))
        gt.append(_pose(Rc @ R0.T, cg[i]))
    return dict(est=np.array(est), gt=np.array(gt), centres_est=c, centres_gt=cg, good=good, inliers=good, src=c.astype(np.float32),
                dst=cg.astype(np.float32), s=s, R=R0, t=t0)


def problems():
    """name -> (scene dict, search keywords) of every search the GPU tests compare with the model"""
    P = {"n3": (cloud(3, 3, seed=1), {}), "n4": (cloud(4, 4, seed=2), {})}
    for n in STRIDE_NS:
        P["stride%d" % n] = (stride_scene(n), {})
    P["rounds"] = (rounds_scene(), {})
    P["capped"] = (rounds_scene(), dict(max_iters=100))
    P["rigid"] = (cloud(80, 60, seed=11, s=1.0), dict(with_scale=False))
    P["rigid_on_scale2"] = (cloud(80, 60, seed=12, s=2.0, box=0.15), dict(with_scale=False))
    P["mirrored"] = (cloud(60, 60, seed=13, mirror=True), {})
    P["planar"] = (cloud(80, 60, seed=14, planar=True), {})
    P["collinear_consensus"] = (collinear_consensus(), dict(thr=0.5, seed=COLLINEAR_SEED))
    P["nan_rows"] = (nan_scene(), {})
    for i, s in enumerate(batch_scenes()):
        P["batch%d" % i] = (s, {})
    P["landmarks"] = (landmark_scene(), {})
    P["trajectory_robust"] = (trajectory_scene(outliers=5), {})
    return {k: (s, dict(dict(thr=THR, seed=SEARCH_SEED), **kw)) for k, (s, kw) in P.items()}
