"""numpy model of the fundamental-matrix search (csrc/vo_fundamental.hip: seven-point RANSAC, eight-point re-fit), the ground truths of the
scenes, and the bounds the library is held to.

Plain numpy, float64 / longdouble and LAPACK; no GPU.  It shares no numerical step with the kernel (elimination with complete pivoting, a
closed-form cubic with Newton steps, Jacobi eigenvectors of the 9 x 9 Gram matrix):

  sample7        the documented draw of hypothesis h (the generator of the other searches, seven draws); no subset check, as OpenCV has none
  seven_point    Hartley normalisation, the null space of the 7 x 9 system from LAPACK's SVD, the homogeneous cubic det(a V1 + b V2) = 0 in
                 the chart (of eight) whose point at infinity has the largest determinant, roots from numpy's companion matrix, denormalised,
                 unit Frobenius norm, the entry of the largest magnitude positive.  Its own truth: each root carried to longdouble by Newton
                 steps on the nine equations (seven epipolar rows, det F = 0, |F| = 1) with longdouble residuals
  err            OpenCV's FMEstimatorCallback::computeError in float64, the same expressions as the kernel, and err_band: how far err may move
                 when the entries of a unit-norm F move by delta
  search         the whole search restated: rounds of 256, most inliers, ties to the smallest h and between the roots of one sample to the
                 smaller sum of err, RANSACUpdateNumIters with 7 model points -- and `decided`: whether a solver whose every model lies within
                 SOLVE_FACTOR x 2^-52 x kappa of this model's must return the same winner, count, mask and number of hypotheses
  eight_point    the normalised eight-point algorithm on a consensus set by SVD of the m x 9 matrix (and by LAPACK's eigh of the Gram matrix,
                 the route whose rounding the kernel shares), the smallest singular value of the 3 x 3 set to zero; truth in longdouble
  ground truth   K^-T [t]x R K^-1

Every bound has the form FACTOR x u x kappa.  FACTOR is 8 x the worst ratio of this float64 model to its own longdouble truth (for the ground
truth: of the model's re-fit to the ground truth), measured by tests/test_fundamental_model.py over the samples the tests use and never on
the kernel: a kernel that eliminates in another order is still backward stable but may lose a few more bits.
"""
import math

import numpy as np

import essential_model as em
import homography_model as hm

K, bits_equal = em.K, em.bits_equal
widen, hartley, splitmix64 = hm.widen, hm.hartley, hm.splitmix64
EPS, LD, BATCH, GT_U = hm.EPS, hm.LD, 256, hm.GT_U
THRESHOLD, CONFIDENCE, MAX_ITERS = 3.0, 0.99, 1000
RANK_TOL = 1e-12                  # s7 / s1 of the normalised 7 x 9 system under this: more than two null dimensions, no model
IMAG_REAL = 1e-8                  # a complex pair with |im| <= IMAG_REAL max(1, |re|) is a double root and kept (twice)
AMBIGUOUS = 100.0                 # a sample within this factor of either tolerance may be judged otherwise by a correct solver: search()
#                                   then reports the search as not decided
SCENES = ("general", "forward", "sideways", "small_baseline", "wide", "plane_off", "noisy")
EXACT = ("general", "forward", "sideways", "wide", "plane_off")       # noise-free scenes with a baseline that holds every point
SEARCH_SEED = 7                   # the search seed of the GPU tests
FULL_SEED = 2                     # scene seed of the full problems (essential_model.FULL_SEED)
# The problems of the GPU tests.  Each is `decided` in the model's own search (search() below) with a winner under KAPPA_CUT, so that the
# library must return the same winner, count, mask and number of hypotheses; tests/test_fundamental_model.py asserts it for every one.
# Where SEARCH_SEED does not give that, the first search seed above it that does is recorded here (small_baseline n = 200: another root of
# the winning sample could reach 200 within its band; plane_off n = 40: the first sample lies on the plane, kappa 2.9e8).
FULL_NS = (40, 200)
FULL_SEARCH_SEEDS = {("small_baseline", 200): 9, ("plane_off", 40): 10}
# loop edges: the lane, wave and workgroup strides of the score and finish kernels, and both sides of cv2's LMedS switch at 15.  Scene:
# `general` with 20 % gross outliers from n = 14 up; scene seed 1, or the first above it with which the search is decided
EDGE_NS = (7, 8, 14, 15, 63, 64, 65, 255, 256, 257)
EDGE_SCENE_SEEDS = {63: 2, 256: 2}
# the batch of three that stop in different rounds: (outlier fraction, scene seed) of `general` at n = 200 -> 256, 512 and 1024 hypotheses
BATCH_SCENES = ((0.0, 11), (0.45, 12), (0.55, 12))
BATCH_ROUNDS = (256, 512, 1024)
# `general` at n = 200 with 30 % gross outliers whose consensus set is the same under the search seeds 3 and 4 (both decided, different
# winners): the first scene seed from 5 up for which the model says so (with 5 an outlier lies 3 px from its line; with 6 seed 3 is not decided)
TWO_SEEDS_SCENE_SEED = 7

# ---- measured constants ---------------------------------------------------------------------------------------------------------------
# tests/test_fundamental_model.py measures each ratio again on the model alone, prints it, and asserts that each factor is 8 x the recorded
# ratio (rounded up) and that the fresh measurement lies within a factor of two of the record.
#
# |F0 - seven_point(sample)| <= SOLVE_FACTOR x 2^-52 x kappa, kappa = s1 / s9 of the 9 x 9 Jacobian of the nine equations at the root in the
# normalised frame (it grows with the conditioning of the null space and with the closeness of two roots of the cubic alike).
SOLVE_FACTOR = 228.0
# a model over this kappa is not compared (its band in search() is as wide as the bound makes it)
KAPPA_CUT = 1e6
# |F - eight_point by eigh| <= REFIT_FACTOR x 2^-52 x kappa2, kappa2 = s1^2 / (s8^2 - s9^2) of the normalised m x 9 matrix
REFIT_FACTOR = 3.7
# |F - F_gt| <= GT_FACTOR x 2^-14 px x kappa8, kappa8 = s1 / s8 of the normalised m x 9 matrix, on the exact scenes
GT_FACTOR = 5.1e-4
# sigma3 / sigma1 of the returned re-fit <= RANK2_FACTOR x 2^-52
RANK2_FACTOR = 0.0175
MEASURED = dict(solve=28.40, refit=0.4576, gt=6.337e-5, rank2=2.183e-3)


# =========================================================================================================================================
# scenes
# =========================================================================================================================================
def scene(name, n=40, seed=FULL_SEED):
    """essential_model.scene, and `plane_off`: its plane with the last max(3, n // 8) points moved 3 .. 10 m off the plane"""
    if name != "plane_off":
        return em.scene(name, n, seed)
    s = dict(em.scene("plane", n, seed))
    rng = np.random.default_rng([seed, 777])
    X = s["X"].copy()
    k = max(3, n // 8)
    X[n - k:, 2] += rng.uniform(3, 10, k) * rng.choice([-1.0, 1.0], k)
    p1 = X @ K.T
    p2 = (X @ s["R"].T + s["t"]) @ K.T
    s.update(name="plane_off", X=X, p1=(p1[:, :2] / p1[:, 2:3]).astype(np.float32), p2=(p2[:, :2] / p2[:, 2:3]).astype(np.float32))
    return s


def with_outliers(name, n, frac, seed):
    """a noise-free scene with int(frac n) of its points moved by 10 +- 60 px in view 2 -> scene dict with `outliers`"""
    s = dict(scene(name, n, seed))
    rng = np.random.default_rng([seed, 99])
    out = np.sort(rng.choice(n, int(frac * n), replace=False))
    p2 = s["p2"].copy()
    p2[out] += (rng.uniform(-60, 60, (len(out), 2)) + 10).astype(np.float32)
    s.update(p2=p2, outliers=out, name="%s+%d%%" % (name, round(100 * frac)))
    return s


def full_search_seed(name, n):
    return FULL_SEARCH_SEEDS.get((name, n), SEARCH_SEED)


def edge_scene(n):
    return with_outliers("general", n, 0.2 if n >= 14 else 0.0, EDGE_SCENE_SEEDS.get(n, 1))


def batch_scenes():
    return [with_outliers("general", 200, frac, seed) for frac, seed in BATCH_SCENES]


def unit(F):
    """unit Frobenius norm, the entry of the largest magnitude positive"""
    F = np.asarray(F)
    F = F / np.sqrt((F * F).sum())
    k = np.unravel_index(np.argmax(np.abs(F)), F.shape)
    return -F if F[k] < 0 else F


def ground_truth(s):
    """the fundamental matrix of a scene dict -> (3, 3) unit; None without a baseline"""
    if s["E_gt"] is None:
        return None
    Ki = np.linalg.inv(s["K"])
    return unit(Ki.T @ s["E_gt"] @ Ki)


def same_F(a, b):
    """max entry of the smaller of a - b and a + b for two unit-norm matrices (F is defined up to sign)"""
    return hm.same_H(a, b)


# =========================================================================================================================================
# sampling
# =========================================================================================================================================
def sample7(seed, h, n):
    """seven distinct indices in [0, n) of hypothesis h: draw k is splitmix64(seed, h, k) mod n, repeats are skipped"""
    idx, k = [], 0
    while len(idx) < 7:
        r = splitmix64(((seed & 0xFFFFFF) << 40) ^ ((h & 0xFFFFFFFF) << 8) ^ (k & 0xFF)) if k < 256 else splitmix64(k)
        i = int((r >> 11) % n)
        k += 1
        if i not in idx:
            idx.append(i)
    return idx


# =========================================================================================================================================
# the minimal solve
# =========================================================================================================================================
def epi_rows(q1, q2):
    """(m, 9): (u x, u y, u, v x, v y, v, x, y, 1) for x2^T F x1 = 0, in the dtype of the points"""
    x, y, u, v = q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1]
    return np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], 1)


def _cof(M):
    """cofactor matrix: d det / d M"""
    return np.array([[M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1], M[1, 2] * M[2, 0] - M[1, 0] * M[2, 2], M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]],
                     [M[0, 2] * M[2, 1] - M[0, 1] * M[2, 2], M[0, 0] * M[2, 2] - M[0, 2] * M[2, 0], M[0, 1] * M[2, 0] - M[0, 0] * M[2, 1]],
                     [M[0, 1] * M[1, 2] - M[0, 2] * M[1, 1], M[0, 2] * M[1, 0] - M[0, 0] * M[1, 2], M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]]], M.dtype)


def _det(M):
    return (M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0])) + \
        M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0])


def denormalise(Fn, c1, s1, c2, s2):
    """T2^T Fn T1, unit"""
    dtype = Fn.dtype.type
    return unit(hm._T(c2, s2, dtype).T @ Fn @ hm._T(c1, s1, dtype))


def _system(f, A):
    """the nine equations at f (9,): A f, det F, (|f|^2 - 1) / 2 -> residual (9,), Jacobian (9, 9), in the dtype of f"""
    Fm = f.reshape(3, 3)
    g = np.concatenate([A @ f, [_det(Fm)], [((f * f).sum() - 1) / 2]])
    J = np.concatenate([A, _cof(Fm).reshape(1, 9), f[None]], 0)
    return g, J


def _polish_ld(f0, A_ld, iters=10):
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no wider than float64 here"
    f = np.asarray(f0, LD)
    for _ in range(iters):
        g, J = _system(f, A_ld)
        d = np.linalg.lstsq(J.astype(np.float64), -g.astype(np.float64), rcond=None)[0]
        f = f + d.astype(LD)
        if np.abs(d).max() <= 1e-19:
            break
    return f / np.sqrt((f * f).sum())


_ANGLES = np.arange(8) * (math.pi / 8)


def seven_point(p1, p2, truth=False):
    """p1, p2 (7, 2) pixels -> dict models (list of dict F (3, 3) float64 unit, kappa, t [truth: F_ld, ratio = |F - F_ld| / (2^-52 kappa)]),
    rank (s7 / s1), ambiguous (a tolerance was met within AMBIGUOUS)"""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    out = dict(models=[], rank=0.0, ambiguous=False)
    if not (np.all(np.isfinite(p1)) and np.all(np.isfinite(p2))):
        return out
    with np.errstate(all="ignore"):
        c1, s1, q1 = hartley(p1)
        c2, s2, q2 = hartley(p2)
        A = epi_rows(q1, q2)
        if not np.all(np.isfinite(A)):
            return out
        _, s, Vt = np.linalg.svd(A)
    out["rank"] = float(s[6] / s[0]) if s[0] > 0 else 0.0
    out["ambiguous"] = bool(RANK_TOL / AMBIGUOUS < out["rank"] < RANK_TOL * AMBIGUOUS)
    if not out["rank"] > RANK_TOL:
        return out
    V1, V2 = Vt[7].reshape(3, 3), Vt[8].reshape(3, 3)
    dets = [abs(_det(math.cos(a) * V1 + math.sin(a) * V2)) for a in _ANGLES]
    a = _ANGLES[int(np.argmax(dets))]
    Q, P = math.cos(a) * V1 + math.sin(a) * V2, -math.sin(a) * V1 + math.cos(a) * V2
    coef = [_det(Q), (_cof(Q) * P).sum(), (_cof(P) * Q).sum(), _det(P)]              # det(P + t Q), highest power first
    if not coef[0] != 0:
        return out
    ts = []
    for r in np.roots(coef):
        rel = abs(r.imag) / max(1.0, abs(r.real))
        if r.imag != 0 and IMAG_REAL / AMBIGUOUS < rel < IMAG_REAL * AMBIGUOUS:
            out["ambiguous"] = True
        if rel <= IMAG_REAL:
            ts.append(float(r.real))
    if truth:
        l1, l2 = hartley(np.asarray(p1, LD), LD), hartley(np.asarray(p2, LD), LD)
        A_ld = epi_rows(l1[2], l2[2])
    for t in ts:
        Fn = P + t * Q
        Fn = Fn / np.sqrt((Fn * Fn).sum())
        sv = np.linalg.svd(_system(Fn.reshape(9), A)[1], compute_uv=False)
        m = dict(F=denormalise(Fn, c1, s1, c2, s2), kappa=float(sv[0] / sv[8]) if sv[8] > 0 else math.inf, t=t)
        if not np.all(np.isfinite(m["F"])):
            return dict(models=[], rank=out["rank"], ambiguous=out["ambiguous"])
        if truth:
            f = _polish_ld(Fn.reshape(9), A_ld)
            m["F_ld"] = denormalise(f.reshape(3, 3), l1[0], l1[1], l2[0], l2[1])
            e = m["F"].astype(LD)
            m["ratio"] = float(min(np.abs(e - m["F_ld"]).max(), np.abs(e + m["F_ld"]).max())) / (EPS * m["kappa"])
        out["models"].append(m)
    return out


def tie_scene(seed=1):
    """eight points on which the tie rule decides: seven points of `general` whose sample has three roots, and an eighth whose view-2
    point is put 0.6, 0.3 px beside the crossing of its epipolar lines under the two best-conditioned roots, so that both roots hold all
    eight points and only the sum of err tells them apart -> scene dict (None if the seed has no such crossing inside the image)"""
    s = dict(scene("general", 8, seed))
    P1, P2 = widen(s["p1"]), widen(s["p2"])
    m = seven_point(P1[:7], P2[:7])["models"]
    if len(m) != 3:
        return None
    x = np.array([P1[7, 0], P1[7, 1], 1.0])
    a, b = [r["F"] @ x for r in sorted(m, key=lambda r: r["kappa"])[:2]]
    X = np.cross(a, b)
    X = X[:2] / X[2]
    if not (0 <= X[0] <= em.W_IMG and 0 <= X[1] <= em.H_IMG):
        return None
    p2 = s["p2"].copy()
    p2[7] = (X + [0.6, 0.3]).astype(np.float32)
    s.update(p2=p2, name="tie")
    return s


def judge_minimal(F0, p1, p2):
    """a solver's F0 for the seven correspondences p1, p2 -> dict ratio (to the nearest of the model's roots), kappa, ok, excused (no root
    of the model under KAPPA_CUT)"""
    m = seven_point(widen(p1), widen(p2))
    F0 = unit(np.asarray(F0, float).reshape(3, 3))
    best = dict(excused=True, ratio=math.inf, ok=False, kappa=math.inf, roots=len(m["models"]))
    for r in m["models"]:
        if not r["kappa"] <= KAPPA_CUT:
            continue
        ratio = same_F(F0, r["F"]) / (EPS * r["kappa"])
        if ratio < best["ratio"]:
            best = dict(excused=False, ratio=ratio, ok=bool(ratio <= SOLVE_FACTOR), kappa=r["kappa"], roots=len(m["models"]))
    return best


# =========================================================================================================================================
# error, consensus, iteration bound, the whole search
# =========================================================================================================================================
def err_parts(F, p1, p2):
    """-> (e1, e2): the squared distances d1^2 s1 (view 1) and d2^2 s2 (view 2) of OpenCV's computeError, float64, the kernel's expressions"""
    F = np.asarray(F, np.float64).reshape(9)
    p1, p2 = widen(p1), widen(p2)
    x, y, u, v = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    with np.errstate(all="ignore"):
        a2, b2, c2 = (F[0] * x + F[1] * y) + F[2], (F[3] * x + F[4] * y) + F[5], (F[6] * x + F[7] * y) + F[8]
        s2, d2 = 1.0 / (a2 * a2 + b2 * b2), (u * a2 + v * b2) + c2
        a1, b1, c1 = (F[0] * u + F[3] * v) + F[6], (F[1] * u + F[4] * v) + F[7], (F[2] * u + F[5] * v) + F[8]
        s1, d1 = 1.0 / (a1 * a1 + b1 * b1), (x * a1 + y * b1) + c1
        return (d1 * d1) * s1, (d2 * d2) * s2


def err(F, p1, p2):
    """err = max(e1, e2); inf where either is not finite (never an inlier)"""
    e1, e2 = err_parts(F, p1, p2)
    with np.errstate(invalid="ignore"):
        e = np.where(e1 > e2, e1, e2)
    e[~(np.isfinite(e1) & np.isfinite(e2))] = np.inf
    return e


def consensus(F, p1, p2, thr=THRESHOLD):
    e1, e2 = err_parts(F, p1, p2)
    with np.errstate(invalid="ignore"):
        return (e1 <= thr * thr) & (e2 <= thr * thr)


def err_band(F, p1, p2, delta):
    """how far err may move at each point when every entry of the unit-norm F moves by at most delta (and the evaluation itself rounds):
    a line coefficient a = F_r . (x, y, 1) moves by at most delta m, m = |x| + |y| + 1; the numerator d = x2 . l by delta m1 m2; the
    gradient norm g = sqrt(a^2 + b^2) by sqrt 2 delta m.  dist = |d| / g then moves by at most (delta m1 m2 + dist sqrt 2 delta m) /
    (g - sqrt 2 delta m) and err = dist^2 by 2 dist D + D^2; inf where g does not stay positive.  The 16 roundings of the evaluation are
    covered by adding 16 x 2^-52 to delta (each is relative to a term no larger than m1 m2 max|F|, and max|F| <= 1)"""
    F = np.asarray(F, np.float64).reshape(9)
    p1, p2 = widen(p1), widen(p2)
    x, y, u, v = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    delta = delta + 16 * EPS
    with np.errstate(all="ignore"):
        m1, m2 = np.abs(x) + np.abs(y) + 1, np.abs(u) + np.abs(v) + 1
        band = np.zeros(len(x))
        for (a, b, c, mm, px, py) in (((F[0] * x + F[1] * y) + F[2], (F[3] * x + F[4] * y) + F[5], (F[6] * x + F[7] * y) + F[8], m1, u, v),
                                      ((F[0] * u + F[3] * v) + F[6], (F[1] * u + F[4] * v) + F[7], (F[2] * u + F[5] * v) + F[8], m2, x, y)):
            g = np.sqrt(a * a + b * b)
            dist = np.abs((px * a + py * b) + c) / g
            dg = math.sqrt(2.0) * delta * mm
            D = (delta * m1 * m2 + dist * dg) / (g - dg)
            bnd = 2 * dist * D + D * D
            bnd[~(g > dg) | ~np.isfinite(bnd)] = np.inf
            band = np.maximum(band, bnd)
    return band


def ransac_num_iters(conf, outlier_ratio, max_iters=MAX_ITERS):
    return em.ransac_num_iters(conf, outlier_ratio, 7, max_iters)


def hypothesis(p1, p2, seed, h, thr=THRESHOLD):
    """-> (idx, dict of seven_point, list per model of dict cnt, sum, lo, hi): lo / hi bound the count of a solver whose model lies within
    SOLVE_FACTOR x 2^-52 x kappa of this one"""
    n = len(p1)
    idx = sample7(seed, h, n)
    m = seven_point(widen(p1)[idx], widen(p2)[idx])
    rows = []
    for r in m["models"]:
        e = err(r["F"], p1, p2)
        inl = consensus(r["F"], p1, p2, thr)
        band = err_band(r["F"], p1, p2, SOLVE_FACTOR * EPS * r["kappa"])
        with np.errstate(invalid="ignore"):
            lo, hi = int((e + band <= thr * thr).sum()), int((e - band <= thr * thr).sum())
        if m["ambiguous"]:
            lo, hi = 0, n
        rows.append(dict(cnt=int(inl.sum()), sum=float(e[inl].sum()), lo=lo, hi=hi))
    return idx, m, rows


def _pick(rows):
    """the model of one sample: most inliers, then the smaller sum of err, then the first -> index or -1"""
    k = -1
    for i, r in enumerate(rows):
        if k < 0 or r["cnt"] > rows[k]["cnt"] or (r["cnt"] == rows[k]["cnt"] and r["sum"] < rows[k]["sum"]):
            k = i
    return k


def search(p1, p2, thr=THRESHOLD, conf=CONFIDENCE, max_iters=MAX_ITERS, seed=0):
    """the whole search -> dict best (-1: none), hypotheses, F0, mask, count, n_roots, models, kappa (of the winner), decided, why (what
    keeps it from being decided), tie_margin (relative, between the winner and the next root of its sample with the same count; inf if none)"""
    n = len(p1)
    niters, h_done, best, best_count, F0, n_roots, models, kappa = max_iters, 0, -1, 6, None, 0, 0, math.inf
    decided, why, tie_margin = True, [], math.inf
    max_lo, max_hi, seen = 6, 6, []
    while True:
        for h in range(h_done, h_done + BATCH):
            _, m, rows = hypothesis(p1, p2, seed, h, thr)
            models += len(rows)
            if m["ambiguous"]:
                decided = False
                why.append("sample %d is within %g of a tolerance" % (h, AMBIGUOUS))
            k = _pick(rows)
            for r in rows:
                max_lo, max_hi = max(max_lo, r["lo"]), max(max_hi, r["hi"])
            seen.append((h, k, rows))
            if k >= 0 and rows[k]["cnt"] > best_count:
                best, best_count, F0, n_roots, kappa = h, rows[k]["cnt"], m["models"][k]["F"], len(rows), m["models"][k]["kappa"]
        h_done += BATCH
        if max_lo != max_hi:                                    # the running best's count decides the bound of this round
            decided = False
            why.append("after %d hypotheses the best count lies in %d .. %d" % (h_done, max_lo, max_hi))
        if best >= 0:
            niters = min(niters, ransac_num_iters(conf, (n - best_count) / n, max_iters))
        if h_done >= niters:
            break
    if best >= 0:
        for h, k, rows in seen:
            for i, r in enumerate(rows):
                if h == best and i == k:
                    if r["lo"] != r["hi"]:
                        decided = False
                        why.append("the winner's count lies in %d .. %d" % (r["lo"], r["hi"]))
                elif h == best:
                    if r["hi"] >= best_count:
                        if r["lo"] == r["hi"] == best_count:
                            tie_margin = min(tie_margin, abs(r["sum"] - rows[k]["sum"]) / max(r["sum"], rows[k]["sum"], 1e-300))
                        else:
                            decided = False
                            why.append("another root of the winning sample may reach %d" % r["hi"])
                elif r["hi"] > best_count or (h < best and r["hi"] == best_count):
                    decided = False
                    why.append("hypothesis %d may reach %d" % (h, r["hi"]))
        if tie_margin <= 1e-6:
            decided = False
            why.append("the tie between two roots has a margin of %.3g" % tie_margin)
    mask = consensus(F0, p1, p2, thr) if best >= 0 else np.zeros(n, bool)
    return dict(best=best, hypotheses=h_done, F0=F0, mask=mask, count=best_count if best >= 0 else 0, n_roots=n_roots, models=models,
                kappa=kappa, decided=decided, why=why, tie_margin=tie_margin)


# =========================================================================================================================================
# the eight-point re-fit
# =========================================================================================================================================
def _rank2(Fn):
    U, s, Vt = np.linalg.svd(Fn)
    return (U[:, :2] * s[:2]) @ Vt[:2]


def sigma3_rel(F):
    """sigma3 / sigma1 of a 3 x 3, sigma3 = |det| / (sigma1 sigma2) with the determinant in longdouble (LAPACK's own sigma3 is only good to
    2^-52 sigma1)"""
    F = np.asarray(F, np.float64).reshape(3, 3)
    s = np.linalg.svd(F, compute_uv=False)
    return float(abs(_det(F.astype(LD))) / (s[0] * s[1]) / s[0])


def eight_point(p1, p2, mask, truth=False):
    """normalised eight-point algorithm on the correspondences of `mask` -> dict F (SVD of the m x 9 matrix, rank 2), F_eigh (LAPACK eigh of
    the Gram matrix, rank 2), kappa2 = s1^2 / (s8^2 - s9^2), kappa8 = s1 / s8; [truth: F_ld, ratio_eigh = |F_eigh - F_ld| / (2^-52 kappa2)]"""
    a, b = widen(p1)[mask], widen(p2)[mask]
    c1, s1, q1 = hartley(a)
    c2, s2, q2 = hartley(b)
    A = epi_rows(q1, q2)
    _, s, Vt = np.linalg.svd(A)
    s9 = s[8] if len(s) > 8 else 0.0
    lam, V = np.linalg.eigh(A.T @ A)
    out = dict(F=denormalise(_rank2(Vt[8].reshape(3, 3)), c1, s1, c2, s2), F_eigh=denormalise(_rank2(V[:, 0].reshape(3, 3)), c1, s1, c2, s2),
               kappa2=float(s[0] ** 2 / (s[7] ** 2 - s9 ** 2)), kappa8=float(s[0] / s[7]))
    if truth:
        l1, l2 = hartley(np.asarray(a, LD), LD), hartley(np.asarray(b, LD), LD)
        A_ld = epi_rows(l1[2], l2[2])
        M = A_ld.T @ A_ld
        h = Vt[8].astype(LD)
        for _ in range(40):                                   # inverse iteration on the longdouble Gram matrix, longdouble residuals
            mu = h @ (M @ h)
            g = M @ h - mu * h
            B = (M - mu * np.eye(9, dtype=LD)).astype(np.float64)
            Mx = np.concatenate([np.concatenate([B, -h.astype(np.float64)[:, None]], 1), np.concatenate([h.astype(np.float64), [0.0]])[None]], 0)
            d = np.linalg.lstsq(Mx, np.concatenate([-g.astype(np.float64), [0.0]]), rcond=None)[0][:9]
            h = h + d.astype(LD)
            h = h / np.sqrt((h * h).sum())
            if np.abs(d).max() <= 1e-19:
                break
        # rank 2 in longdouble: the right singular vector w of sigma3 from LAPACK, refined as the null direction of Fn^T Fn - sigma3^2
        Fn = h.reshape(3, 3)
        w = np.linalg.svd(Fn.astype(np.float64))[2][2].astype(LD)
        G = Fn.T @ Fn
        for _ in range(20):
            mu = w @ (G @ w)
            g = G @ w - mu * w
            B = (G - mu * np.eye(3, dtype=LD)).astype(np.float64)
            Mx = np.concatenate([np.concatenate([B, -w.astype(np.float64)[:, None]], 1), np.concatenate([w.astype(np.float64), [0.0]])[None]], 0)
            d = np.linalg.lstsq(Mx, np.concatenate([-g.astype(np.float64), [0.0]]), rcond=None)[0][:3]
            w = w + d.astype(LD)
            w = w / np.sqrt((w * w).sum())
            if np.abs(d).max() <= 1e-19:
                break
        Fn = Fn - np.outer(Fn @ w, w)
        out["F_ld"] = denormalise(Fn, l1[0], l1[1], l2[0], l2[1])
        e = out["F_eigh"].astype(LD)
        out["ratio_eigh"] = float(min(np.abs(e - out["F_ld"]).max(), np.abs(e + out["F_ld"]).max())) / (EPS * out["kappa2"])
    return out


def cost(F, p1, p2, mask):
    """sum of err over `mask` at F"""
    return float(err(F, p1, p2)[mask].sum())


def judge_refit(F, cost_got, p1, p2, mask):
    """a solver's refit = 1 answer and cost on the correspondences of `mask` -> dict ratio (against eigh of the same Gram matrix), ok, kappa2,
    kappa8, rank2 (sigma3 / sigma1 / 2^-52), rank2_ok, cost_model, cost_slack (what the bound on F lets the cost move), cost_ok"""
    f = eight_point(p1, p2, mask)
    Fu = unit(np.asarray(F, float).reshape(3, 3))
    ratio = same_F(Fu, f["F_eigh"]) / (EPS * f["kappa2"])
    slack = float(err_band(f["F_eigh"], p1, p2, REFIT_FACTOR * EPS * f["kappa2"])[mask].sum())
    cm = cost(f["F_eigh"], p1, p2, mask)
    r2 = sigma3_rel(Fu) / EPS
    return dict(ratio=ratio, ok=bool(ratio <= REFIT_FACTOR), kappa2=f["kappa2"], kappa8=f["kappa8"], rank2=r2, rank2_ok=bool(r2 <= RANK2_FACTOR),
                cost_model=cm, cost_slack=slack, cost_ok=bool(cost_got <= cm + slack), model=f)


def judge_gt(F, s, kappa8):
    """-> dict ratio = |F - F_gt| / (2^-14 kappa8), ok"""
    ratio = same_F(unit(np.asarray(F, float).reshape(3, 3)), ground_truth(s)) / (GT_U * kappa8)
    return dict(ratio=ratio, ok=bool(ratio <= GT_FACTOR))


def essential_defect(F, Kc=K):
    """K^T F K of a calibrated pair is an essential matrix: -> ((sigma1 - sigma2) / sigma1, sigma3 / sigma1)"""
    s = np.linalg.svd(Kc.T @ np.asarray(F, float).reshape(3, 3) @ Kc, compute_uv=False)
    return float((s[0] - s[1]) / s[0]), float(s[2] / s[0])


def essential_defect_slack(F, delta, Kc=K):
    """how far either figure of essential_defect may move when the entries of the unit-norm F move by delta: the singular values of
    K^T F K by at most |K^T dF K|_2 <= 3 delta |K|_2^2, and each figure is a difference of two of them over sigma1"""
    s = np.linalg.svd(Kc.T @ np.asarray(F, float).reshape(3, 3) @ Kc, compute_uv=False)
    return float(4 * 3 * delta * np.linalg.norm(Kc, 2) ** 2 / s[0])
