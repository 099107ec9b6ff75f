"""numpy model of the 2D-2D bootstrap pose (csrc/vo_essential.hip: five-point RANSAC + recoverPose), its scenes and the bounds it is held to.

Plain numpy, float64 / longdouble and LAPACK; no GPU and no oracle.  It shares no step with Nister's chain of the kernel and of
oracle/essential_oracle.py (complete-pivot null space, Gauss-Jordan, 10th-degree determinant, bisection, cross-product back-substitution,
one-sided Jacobi), so a weakness the two have in common shows up against it.

  minimal solver  null space of the 5 x 9 epipolar system from LAPACK's SVD; the ten cubics det E = 0, 2 E E^T E - tr(E E^T) E = 0 by plain
                  polynomial arithmetic on (4, 4, 4) coefficient arrays; the 10 x 10 action matrix of a fixed linear form on the quotient
                  ring (Stewenius, Engels, Nister 2006) and its eigenvectors -> ten complex candidates.
  certification   every candidate's real part is polished by Gauss-Newton on the FULL system in the nine entries of E (5 epipolar rows,
                  the 9 + 1 cubics, |E|^2 = 1), residuals in longdouble.  A root is certified when its float64 residuals are within
                  RES_EPI_MAX and RES_CUB_MAX; nothing else is ever used as an expectation.  Real candidates that fail are reported.
  conditioning    sigma = smallest singular value of that 16 x 9 Jacobian at the root.  A backward-stable solver's E is off by a modest
                  multiple of 2^-52 / sigma; a perturbation d of the data moves the root by about |d| / sigma.
  sixth point     a correspondence generated from a certified root, rounded to float32 pixels, with the Sampson distance the rounding left.
  validity        (s1 - s2) / s1 and s3 / s1 of LAPACK's singular values; float64 Sampson distances in pixels.
  pose            the four (R, t) of LAPACK's SVD as a SET, LAPACK triangulation of every inlier, the reference's three rules, and a per-point
                  flag "within the triangulation's own rounding of a rule's threshold".
  iteration bound RANSACUpdateNumIters of OpenCV's ptsetreg.cpp restated.

Every tolerance below carries its derivation or the value measured on the oracle by tests/test_essential_model.py (never on the kernel).
"""
import itertools
import math

import numpy as np

from vo_mi355x import synthetic as syn

K = syn.KITTI_K
F = (K[0, 0] + K[1, 1]) / 2.0
EPS = 2.0 ** -52
LD = np.longdouble
DIST = 50.0                       # recoverPose's distanceThresh as the reference leaves it
BATCH = 256                       # hypotheses per round of the library
W_IMG, H_IMG = 1241.0, 376.0

# ---- certification bounds --------------------------------------------------------------------------------------------------------------
# A root polished in longdouble and rounded to float64 is within 2^-53 per entry of an exact root; |E| = 1 and the normalised points are
# below 1.5 in magnitude, so its float64 residuals are a few 2^-53.  Measured over all 164 roots of the root scenes and seeds
# (test_essential_model.py::test_model_certifies_itself): epipolar 1.99e-16, cubic 2.22e-16.  The bounds are those x 4, rounded up.
RES_EPI_MAX = 1e-15
RES_CUB_MAX = 1e-15
IMAG_REAL = 1e-8                  # a candidate whose imaginary part is below this (relative) counts as real: it must certify or is reported

# ---- bounds on a solver's E ------------------------------------------------------------------------------------------------------------
# |E - E_k| <= ROOT_MARGIN x 2^-52 / sigma.  Measured on the oracle (with its Gauss-Newton refinement; without it the worst case was 1.3e11):
# 0.352 over the 164 sixth-point calls, 0.188 over the 32 minimal calls, 0.062 over the 20 judged full problems; worst x 4 = 1.41, rounded up.
ROOT_MARGIN = 1.5
# a root under this sigma is excused (near a double root the first-order scale no longer describes the error); counted, capped at 10 %.
# Measured: 2 of the 164 roots lie under it and 2 of the 164 sixth-point calls are excused (1.2 %)
SIGMA_CUT = 1e-5
EXCUSED_MAX = 0.10
# validity of a 3 x 3 E that is within tol (max entry) of an exact essential matrix E' (singular values 1/sqrt2, 1/sqrt2, 0): Weyl gives
# |s_i(E) - s_i(E')| <= |E - E'|_2 <= 3 tol, hence (s1 - s2) / s1 <= 2 x 3 tol x sqrt2 and s3 / s1 <= 3 tol x sqrt2; both under 9 tol.
# Measured on the oracle: at most 0.061 x 2^-52 / sigma.
VALID_FACTOR = 9.0
# |E - E_gt| on a noise-free scene: the float32 pixels are off by at most 2^-14 px (half an ulp under 2048 px), i.e. d = 2^-14 / F per
# normalised coordinate; an epipolar row kron(x2, x1) moves by at most d (|x1| + |x2|) <= 3 d, the five rows by sqrt5 x 3 d = 6.7 d, the root
# by 6.7 d / sigma to first order.  GT_FACTOR = 16 leaves a factor 2.4 for the second order.  Measured: the model's own roots 0.10 d / sigma,
# the oracle's winners on the full problems at most 0.08 d / sigma.
GT_DELTA = 2.0 ** -14 / F
GT_FACTOR = 16.0
# an E that fits the five points of a certified root E_k within the normalised threshold tn (Sampson distance; its gradient has norm <= 2 |E|)
# and meets the cubics differs from E_k by d with |J d| <= sqrt5 x 2 tn, so |d| <= 4.5 tn / sigma; FIT_FACTOR = 8 covers the second order.
# Measured on the oracle: at most 0.043 tn / sigma.
FIT_FACTOR = 8.0
# consensus: a point whose float64 Sampson distance is within this relative band of the threshold may fall on either side (the kernel sums
# the nine products in another order: a few 2^-52, amplified by the cancellation in x2^T E x1 of a near-inlier); at most BAND_POINTS per
# problem.  Measured on the oracle: no point differs, none lies in the band.
BAND_REL = 1e-9
BAND_POINTS = 2


def outlier_leak(n):
    """gross outliers (moved by 10 +- 60 px) that may sit in the consensus set: one lands within 1 px of its epipolar line with probability
    about 2 / 70, and the winner was chosen for holding many points; the bound is the one tests/test_gpu_essential.py has always used"""
    return 0.03 * n + 2
# rounding of the triangulated point relative to the gap of its 4 x 4 system: 64 x 2^-52 x s1 / (s3 - s4).  Measured: no point is flagged.
NEAR_FACTOR = 64.0
POSE_TOL = 1e-9                   # |det R - 1|, ||t| - 1| as the issue states them
# returned (R, t) against a candidate of LAPACK's decomposition of the same E: the two singular vectors of the double singular value are
# free, the products U W V^T and u3 are not; their error is a few 2^-52 / (relative gap to s3 = 1).  The oracle decomposes with LAPACK too
# (measured 0); 1e-12 leaves four digits to a Jacobi SVD.
CAND_TOL = 1e-12
# sixth-point calls won by a later hypothesis than the first (the first drew a subset whose root does not hold the sixth point within the
# threshold).  Measured on the oracle: 0 of 164, and the kernel runs the same search, so none is allowed.
LATE_MAX = 0
# on a four-way tie the returned rotation against the true one: the search accepts the first E that holds every point within 1 px, an angle
# of 1 / F = 1.4e-3, and does not refit, so R is off by a small multiple of that; 1e-2 is the existing suite's bound on R at this threshold
# (test_gpu_essential.py) and still 200 times under the distance to the twisted pair.  Measured over search seeds 7, 8, 9: at most 1.1e-4.
TIE_R_TOL = 1e-2

SCENES = ("general", "forward", "sideways", "sideways_rot", "big_rotation", "plane", "fronto", "pure_rotation", "small_baseline", "wide", "noisy")
ROOT_SCENES = ("general", "forward", "sideways", "sideways_rot", "big_rotation", "plane", "fronto", "wide")
ROOT_SEEDS = (1, 2, 3, 4)
FULL_SEED = 2                     # scene seed of the full problems: with it no winning sample lies under SIGMA_CUT (with seed 1 `general` n = 40
#                                   and `plane` n = 200 did and were excused); pure_rotation always does, its five-point system is singular
TIE_SEEDS = (4, 5, 17, 24, 41, 9) # search seeds of the n = 5 tie calls: the first five draw the five points in the same order as hypothesis 0
#                                   (hence bit-equal E), the sixth in another
PLANAR = ("plane", "fronto")
NO_BASELINE = ("pure_rotation", "small_baseline")
_MOTION = dict(                   # rvec, t (metres; depths are 8 .. 45 m)
    general=((0.02, -0.04, 0.01), (0.7, 0.2, -0.6)),
    forward=((0.005, 0.01, -0.002), (0.02, -0.01, -1.0)),
    sideways=((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)),
    sideways_rot=((0.0, -0.05, 0.01), (1.0, 0.05, 0.1)),
    big_rotation=((0.1, -0.45, 0.15), (0.8, 0.1, -0.3)),
    plane=((0.01, 0.03, -0.005), (0.6, 0.1, -0.5)),
    fronto=((0.0, 0.02, 0.0), (1.0, 0.0, 0.0)),
    pure_rotation=((0.01, 0.03, -0.005), (0.0, 0.0, 0.0)),
    small_baseline=((0.01, 0.03, -0.005), (0.056, 0.016, -0.048)),      # |t| = 0.0755 < 1 % of the nearest depth (8 m)
    wide=((0.02, -0.04, 0.01), (0.7, 0.2, -0.6)),
    noisy=((0.02, -0.04, 0.01), (0.7, 0.2, -0.6)),
)


# =========================================================================================================================================
# scenes
# =========================================================================================================================================
def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def scene(name, n=40, seed=1):
    """-> dict name, K, p1, p2 (n, 2) float32 pixels, R, t (metres), E_gt (unit norm, None without a baseline), X (n, 3), outliers (indices)"""
    rng = np.random.default_rng([seed, SCENES.index(name)])
    rvec, t = _MOTION[name]
    R, t = syn.rodrigues(np.asarray(rvec, float)), np.asarray(t, float)
    X = np.stack([rng.uniform(-15, 15, n), rng.uniform(-3, 3, n), rng.uniform(8, 45, n)], 1)
    if name == "plane":
        X[:, 2] = 22.0 + 0.5 * X[:, 0] + 0.3 * X[:, 1]
    elif name == "fronto":
        X[:, 2] = 20.0
    elif name == "wide":                                  # the four image corners and the principal point first, the rest anywhere in the image
        px = np.stack([rng.uniform(0, W_IMG, n), rng.uniform(0, H_IMG, n)], 1)
        fixed = np.array([[0, 0], [W_IMG, 0], [0, H_IMG], [W_IMG, H_IMG], [K[0, 2], K[1, 2]]])
        px[:min(n, 5)] = fixed[:min(n, 5)]
        X[:, 0], X[:, 1] = (px[:, 0] - K[0, 2]) / K[0, 0] * X[:, 2], (px[:, 1] - K[1, 2]) / K[1, 1] * X[:, 2]
    p1 = X @ K.T
    p1 = p1[:, :2] / p1[:, 2:3]
    if name == "wide":
        p1 = px                                           # the corners to the bit (the projection of X returns them within 1e-13 px)
    Xc = X @ R.T + t
    p2 = Xc @ K.T
    p2 = p2[:, :2] / p2[:, 2:3]
    out = np.zeros(0, int)
    if name == "noisy":
        p1 = p1 + rng.normal(0, 0.3, p1.shape)
        p2 = p2 + rng.normal(0, 0.3, p2.shape)
        out = np.sort(rng.choice(n, int(0.3 * n), replace=False))
        p2[out] += rng.uniform(-60, 60, (len(out), 2)) + 10
    E_gt = None
    if np.linalg.norm(t) > 0:
        E_gt = skew(t) @ R
        E_gt = E_gt / np.linalg.norm(E_gt)
    return dict(name=name, K=K, p1=p1.astype(np.float32), p2=p2.astype(np.float32), R=R, t=t, E_gt=E_gt, X=X, outliers=out)


def normalise(p, Kc=K):
    """float32 pixels widened to float64 (exact), then (p - c) / f as the library does"""
    p = np.asarray(p, np.float32).astype(np.float64).reshape(-1, 2)
    return np.stack([(p[:, 0] - Kc[0, 2]) / Kc[0, 0], (p[:, 1] - Kc[1, 2]) / Kc[1, 1]], 1)


def epipolar_rows(q1, q2, dtype=np.float64):
    """[n, 9]: row i is kron(x2_i, x1_i), so that row . vec(E) = x2^T E x1 with E row-major"""
    x1 = np.concatenate([np.asarray(q1, dtype), np.ones((len(q1), 1), dtype)], 1)
    x2 = np.concatenate([np.asarray(q2, dtype), np.ones((len(q2), 1), dtype)], 1)
    return (x2[:, :, None] * x1[:, None, :]).reshape(len(x1), 9)


# =========================================================================================================================================
# the full system and its Jacobian
# =========================================================================================================================================
def cubic_residuals(E):
    """[10]: 2 E E^T E - tr(E E^T) E (row-major) and det E, in E's dtype"""
    EEt = E @ E.T
    C = 2 * (EEt @ E) - (EEt[0, 0] + EEt[1, 1] + EEt[2, 2]) * E
    det = E[0, 0] * (E[1, 1] * E[2, 2] - E[1, 2] * E[2, 1]) - E[0, 1] * (E[1, 0] * E[2, 2] - E[1, 2] * E[2, 0]) + \
        E[0, 2] * (E[1, 0] * E[2, 1] - E[1, 1] * E[2, 0])
    return np.concatenate([C.reshape(9), [det]])


def system_residuals(E, A):
    """[m + 11]: epipolar rows, the ten cubics, |E|^2 - 1"""
    e = E.reshape(9)
    return np.concatenate([A @ e, cubic_residuals(E), [e @ e - 1]])


def system_jacobian(E, A):
    """[m + 11, 9] float64"""
    E = np.asarray(E, np.float64)
    EEt, EtE, tr = E @ E.T, E.T @ E, np.trace(E @ E.T)
    J = np.zeros((len(A) + 11, 9))
    J[:len(A)] = A
    for k in range(9):
        D = np.zeros(9)
        D[k] = 1.0
        D = D.reshape(3, 3)
        dC = 2 * (D @ EtE + E @ D.T @ E + EEt @ D) - 2 * np.sum(E * D) * E - tr * D
        J[len(A):len(A) + 9, k] = dC.reshape(9)
        i, j = divmod(k, 3)
        r, c = [x for x in range(3) if x != i], [x for x in range(3) if x != j]
        J[len(A) + 9, k] = (-1) ** (i + j) * (E[r[0], c[0]] * E[r[1], c[1]] - E[r[0], c[1]] * E[r[1], c[0]])
    J[len(A) + 10] = 2 * E.reshape(9)
    return J


def polish(E0, A, iters=12):
    """Gauss-Newton on the full system from E0: residuals and the iterate in longdouble, the step from LAPACK.  -> E float64 (3, 3)"""
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no wider than float64 here"
    A_ld = np.asarray(A, LD)
    E = np.asarray(E0, LD).reshape(3, 3)
    E = E / np.sqrt((E * E).sum())
    for _ in range(iters):
        r = system_residuals(E, A_ld).astype(np.float64)
        if not np.all(np.isfinite(r)):
            break
        step = np.linalg.lstsq(system_jacobian(E.astype(np.float64), A), -r, rcond=None)[0]
        E = E + step.reshape(3, 3).astype(LD)
        if np.abs(step).max() <= 1e-19:
            break
    return E.astype(np.float64)


def residual_maxima(E, A):
    """-> (max |epipolar residual|, max |cubic residual|, ||E|^2 - 1|) in float64"""
    r = system_residuals(np.asarray(E, np.float64), np.asarray(A, np.float64))
    return np.abs(r[:len(A)]).max(), np.abs(r[len(A):len(A) + 10]).max(), abs(r[-1])


def certified(E, A):
    if not np.all(np.isfinite(E)):
        return False
    epi, cub, nrm = residual_maxima(E, A)
    return bool(epi <= RES_EPI_MAX and cub <= RES_CUB_MAX and nrm <= 8 * EPS)


def sigma_min(E, A):
    return float(np.linalg.svd(system_jacobian(E, A), compute_uv=False)[-1])


def same_E(a, b):
    """max entry of the smaller of a - b and a + b (E is defined up to sign)"""
    return float(min(np.abs(a - b).max(), np.abs(a + b).max()))


# =========================================================================================================================================
# minimal solver
# =========================================================================================================================================
def _lin(c):
    """c[0] x + c[1] y + c[2] z + c[3] as a (4, 4, 4) coefficient array, p[i, j, k] of x^i y^j z^k"""
    p = np.zeros((4, 4, 4))
    p[1, 0, 0], p[0, 1, 0], p[0, 0, 1], p[0, 0, 0] = c
    return p


def _mul_lin(p, c):
    """p times the linear polynomial c (the degree never passes 3 here)"""
    out = c[3] * p
    out[1:] += c[0] * p[:-1]
    out[:, 1:] += c[1] * p[:, :-1]
    out[:, :, 1:] += c[2] * p[:, :, :-1]
    return out


_monomials = lambda d: sorted((m for m in itertools.product(range(4), repeat=3) if sum(m) == d), reverse=True)
_DEG3 = _monomials(3)                                                                        # the ten that are eliminated, x^3 first
_BASIS = _monomials(2) + _monomials(1) + _monomials(0)                                       # x^2 xy xz y^2 yz z^2 x y z 1
TRIALS = 3
_FORM = (0.6, -0.5, 0.7)                                                                     # the linear form whose action is diagonalised


def cubic_constraints(N):
    """N (4, 9): E = x N[0] + y N[1] + z N[2] + N[3].  -> ten (4, 4, 4) coefficient arrays"""
    e = [[N[:, 3 * i + j] for j in range(3)] for i in range(3)]
    L = [[_lin(e[i][j]) for j in range(3)] for i in range(3)]
    minor = lambda a, b, c, d: _mul_lin(L[a[0]][a[1]], e[b[0]][b[1]]) - _mul_lin(L[c[0]][c[1]], e[d[0]][d[1]])
    det = _mul_lin(minor((1, 1), (2, 2), (1, 2), (2, 1)), e[0][0]) - _mul_lin(minor((1, 0), (2, 2), (1, 2), (2, 0)), e[0][1]) + \
        _mul_lin(minor((1, 0), (2, 1), (1, 1), (2, 0)), e[0][2])
    EEt = [[sum(_mul_lin(L[i][k], e[j][k]) for k in range(3)) for j in range(3)] for i in range(3)]
    tr = EEt[0][0] + EEt[1][1] + EEt[2][2]
    out = [det]
    for i in range(3):
        for j in range(3):
            out.append(sum(_mul_lin(2 * EEt[i][k], e[k][j]) for k in range(3)) - _mul_lin(tr, e[i][j]))
    return out


def _candidates(N, form):
    """the ten complex solutions (x, y, z) of the cubics of the basis N from the action matrix of `form`; None if the elimination is singular"""
    cons = cubic_constraints(N)
    M = np.array([[c[m] for m in _DEG3 + _BASIS] for c in cons])
    try:
        B = np.linalg.solve(M[:, :10], M[:, 10:])
    except np.linalg.LinAlgError:
        return None
    act = np.zeros((10, 10))
    for var, w in enumerate(form):
        for r, b in enumerate(_BASIS):
            m = tuple(b[i] + (i == var) for i in range(3))
            if m in _DEG3:
                act[r] -= w * B[_DEG3.index(m)]
            else:
                act[r, _BASIS.index(m)] += w
    if not np.all(np.isfinite(act)):
        return None
    _, vec = np.linalg.eig(act)
    return [v[6:9] / v[9] for v in vec.T if abs(v[9]) > 0]


def five_point(q1, q2):
    """q1, q2 (5, 2) normalised points -> dict
         roots        certified essential matrices, unit Frobenius norm (any order, one per real solution)
         sigma        smallest singular value of the full system's Jacobian at each
         uncertified  real candidates (|imag| <= IMAG_REAL) that did not certify -- to be reported, never used
         A            the 5 x 9 system
    The elimination runs in TRIALS random rotations of the null-space basis (a special motion such as R = I can make one chart singular);
    the certified roots of all of them are united.  Certification makes a spurious candidate harmless, the union makes a lost one unlikely."""
    A = epipolar_rows(q1, q2)
    N0 = np.linalg.svd(A)[2][5:]
    rng = np.random.default_rng(55)
    roots, uncertified = [], []
    for trial in range(TRIALS):
        Q = np.linalg.qr(rng.normal(size=(4, 4)))[0]
        N = Q @ N0
        for w in _candidates(N, _FORM) or []:
            E0 = (np.concatenate([w.real, [1.0]]) @ N).reshape(3, 3)
            if not np.all(np.isfinite(E0)) or not np.abs(E0).max() > 0:
                continue
            E = polish(E0, A)
            if certified(E, A):
                if all(same_E(E, r) > 1e-9 for r in roots):
                    roots.append(E)
            elif np.abs(w.imag).max() <= IMAG_REAL * (1 + np.abs(w).max()):
                uncertified.append(E0 / np.linalg.norm(E0))
    uncertified = [U for U in uncertified if all(same_E(U, r) > 1e-6 for r in roots)]
    return dict(roots=roots, sigma=[sigma_min(E, A) for E in roots], uncertified=uncertified, A=A)


def nearest_root(E, q1, q2):
    """the certified root of the five points next to E (Gauss-Newton from E itself) -> (E_k, sigma) or (None, 0.0)"""
    A = epipolar_rows(q1, q2)
    Ek = polish(E, A)
    if not certified(Ek, A):
        return None, 0.0
    return Ek, sigma_min(Ek, A)


def nearest_root_of_subsets(E, q1, q2):
    """over the 5-subsets of (at most 8) points: the certified root next to E with the smallest |E - E_k| sigma -> (ratio to 2^-52, E_k, sigma, subset)"""
    assert len(q1) <= 8
    best = (math.inf, None, 0.0, None)
    for sub in itertools.combinations(range(len(q1)), 5):
        Ek, sg = nearest_root(E, q1[list(sub)], q2[list(sub)])
        if Ek is not None:
            ratio = same_E(E, Ek) * sg / EPS
            if ratio < best[0]:
                best = (ratio, Ek, sg, sub)
    return best


# =========================================================================================================================================
# validity of any E
# =========================================================================================================================================
def validity(E):
    """-> ((s1 - s2) / s1, s3 / s1) of LAPACK's singular values"""
    s = np.linalg.svd(np.asarray(E, float), compute_uv=False)
    return float((s[0] - s[1]) / s[0]), float(s[2] / s[0])


def sampson_px(E, p1, p2, Kc=K):
    """float64 Sampson distance of every correspondence in pixels (normalised distance x (fx + fy) / 2); NaN rows give NaN"""
    q1, q2 = normalise(p1, Kc), normalise(p2, Kc)
    E = np.asarray(E, float)
    with np.errstate(all="ignore"):
        a = [E[r, 0] * q1[:, 0] + E[r, 1] * q1[:, 1] + E[r, 2] for r in range(3)]                  # E x1
        b = [E[0, c] * q2[:, 0] + E[1, c] * q2[:, 1] + E[2, c] for c in range(2)]                  # E^T x2, first two
        num = q2[:, 0] * a[0] + q2[:, 1] * a[1] + a[2]
        return np.abs(num) / np.sqrt(a[0] ** 2 + a[1] ** 2 + b[0] ** 2 + b[1] ** 2) * ((Kc[0, 0] + Kc[1, 1]) / 2.0)


def consensus(E, p1, p2, thr=1.0, Kc=K):
    """-> (mask, band): the float64 mask d <= thr; the points within BAND_REL of the threshold (the only ones a correct solver may flip)"""
    d = sampson_px(E, p1, p2, Kc)
    with np.errstate(invalid="ignore"):
        return d <= thr, np.abs(d - thr) <= BAND_REL * thr


# =========================================================================================================================================
# sixth correspondence
# =========================================================================================================================================
def sixth_point(Ek, seed=0, Kc=K, tries=64):
    """a correspondence of a 3D point under one of the four poses of Ek (spurious roots turn the camera away, so the point may lie behind
    it), rounded to float32 pixels; of `tries` such points the one that rounding moves least off its epipolar line.
    -> (p1 (2,), p2 (2,) float32, the Sampson distance in pixels the rounding left)"""
    rng = np.random.default_rng([seed, 606])
    cands = pose_candidates(Ek)
    best = None
    for _ in range(tries):
        px = np.array([rng.uniform(100, W_IMG - 100), rng.uniform(50, H_IMG - 50)])
        Z = rng.uniform(8, 45)
        X = np.array([(px[0] - Kc[0, 2]) / Kc[0, 0] * Z, (px[1] - Kc[1, 2]) / Kc[1, 1] * Z, Z])
        for R, t in cands:
            Xc = R @ X + t
            if abs(Xc[2]) < 0.2 * np.linalg.norm(Xc):              # either sign of the depth: only the epipolar relation matters here
                continue
            p2 = (Kc @ Xc)[:2] / Xc[2]
            if -1500 <= p2[0] <= W_IMG + 1500 and -1500 <= p2[1] <= H_IMG + 1500:
                p1f, p2f = px.astype(np.float32), p2.astype(np.float32)
                res = float(sampson_px(Ek, p1f[None], p2f[None], Kc)[0])
                if best is None or res < best[2]:
                    best = (p1f, p2f, res)
                break
    if best is None:
        raise RuntimeError("no sixth point")
    return best


# =========================================================================================================================================
# recoverPose
# =========================================================================================================================================
def pose_candidates(E):
    """the four (R, t) of E from LAPACK's SVD; compare as a set"""
    U, _, Vt = np.linalg.svd(np.asarray(E, float))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]])
    Ra, Rb, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
    return [(Ra, t), (Rb, t), (Ra, -t), (Rb, -t)]


def which_candidate(E, R, t):
    """-> (index of the candidate of E next to (R, t), its max entry distance)"""
    d = [max(np.abs(R - Rc).max(), np.abs(t - tc).max()) for Rc, tc in pose_candidates(E)]
    return int(np.argmin(d)), float(min(d))


def cheirality(R, t, q1, q2, dist=DIST):
    """LAPACK triangulation of every correspondence against [I | 0], [R | t] and the reference's rules Q[2] Q[3] > 0, Z < dist, 0 < z2 < dist.
    -> (good [n] bool, near [n] bool: some rule's quantity lies within the triangulation's rounding of its threshold)"""
    n = len(q1)
    A = np.zeros((n, 4, 4))
    A[:, 0, 0], A[:, 0, 2] = -1.0, q1[:, 0]
    A[:, 1, 1], A[:, 1, 2] = -1.0, q1[:, 1]
    A[:, 2, :3], A[:, 2, 3] = q2[:, 0:1] * R[2] - R[0], q2[:, 0] * t[2] - t[0]
    A[:, 3, :3], A[:, 3, 3] = q2[:, 1:2] * R[2] - R[1], q2[:, 1] * t[2] - t[1]
    _, s, Vt = np.linalg.svd(A)
    Q = Vt[:, 3, :]
    with np.errstate(all="ignore"):
        tau = NEAR_FACTOR * EPS * s[:, 0] / (s[:, 2] - s[:, 3])
        c = Q[:, :3] @ R[2] + t[2] * Q[:, 3]                                  # z2 Q[3]
        sg = np.sign(Q[:, 3])
        good = (Q[:, 2] * Q[:, 3] > 0) & ((Q[:, 2] - dist * Q[:, 3]) * sg < 0) & (c * sg > 0) & ((c - dist * Q[:, 3]) * sg < 0)
        near = (np.abs(Q[:, 2]) <= tau) | (np.abs(Q[:, 3]) <= tau) | (np.abs(Q[:, 2] - dist * Q[:, 3]) <= tau * (1 + dist)) | \
            (np.abs(c) <= 2 * tau) | (np.abs(c - dist * Q[:, 3]) <= tau * (2 + dist)) | ~np.isfinite(tau)
    return good, near


def pose_counts(E, q1, q2, dist=DIST):
    """-> [(R, t, good count, near count)] for the four candidates of E"""
    out = []
    for R, t in pose_candidates(E):
        good, near = cheirality(R, t, q1, q2, dist)
        out.append((R, t, int(good.sum()), int(near.sum())))
    return out


def tie_choice(E):
    """the library's documented choice when all four counts are 0: the rotation with the larger trace, then the t with E = +[t]x R.
    -> (R, t); it depends on E alone, not on which singular vector the SVD lists first"""
    cands = pose_candidates(E)
    R = max((c[0] for c in cands[:2]), key=np.trace)
    t = cands[0][1]
    return R, (t if np.sum((skew(t) @ R) * np.asarray(E, float)) > 0 else -t)


def twisted_pair(R, E):
    """the other rotation of E: R_t = R_pi(t) R, a half turn about the baseline"""
    t = pose_candidates(E)[0][1]
    return (2 * np.outer(t, t) - np.eye(3)) @ R


# =========================================================================================================================================
# iteration bound
# =========================================================================================================================================
def ransac_num_iters(prob, outlier_ratio, model_points=5, max_iters=1000):
    """OpenCV's RANSACUpdateNumIters: log(1 - p) / log(1 - (1 - ep)^m), rounded to nearest-even, capped"""
    tiny = np.finfo(float).tiny
    p, ep = min(max(prob, 0.0), 1.0), min(max(outlier_ratio, 0.0), 1.0)
    num = max(1.0 - p, tiny)
    den = 1.0 - (1.0 - ep) ** model_points
    if den < tiny:
        return 0
    num, den = math.log(num), math.log(den)
    if den >= 0 or -num >= max_iters * (-den):
        return max_iters
    return int(round(num / den))


def hypotheses_bounds(n, n_inliers, prob=0.9999, max_iters=1000):
    """-> (lo, hi) for the number of hypotheses the library reports: a multiple of BATCH, at least min(max_iters, N(n_inliers)) and at
    most max_iters rounded up to BATCH"""
    need = min(max_iters, ransac_num_iters(prob, (n - n_inliers) / n, 5, max_iters))
    return need, -(-max_iters // BATCH) * BATCH


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# =========================================================================================================================================
# the problems of the tests and the verdicts on a solver's output (the CPU test applies them to the oracle, the GPU test to the kernel)
# =========================================================================================================================================
# px: the threshold of every sixth-point call, just above what float32 rounding leaves of the sixth correspondence.  Rounding moves a point
# by up to 2.6e-4 px off its epipolar line (half an ulp: 2^-13 px under 4096, 2^-14 px under 2048); sixth_point() keeps the luckiest of 64
# and root_problem() checks that twice its residual stays under the threshold (measured: at most 9.2e-7 px).  So one value serves every call,
# which lets them share one batch, and a root of the same five points that is not E_k has no room to hold the sixth point as well
SIXTH_THR = 1e-5
SAMPSON_ROWS = 30.0               # |x2^T (E - E_k) x1| <= 9 entries x |x2 x1^T| (<= 3.25) x max entry, rounded up
_PROBLEMS = {}


def root_problem(name, seed):
    """five points of a scene, every certified root E_k of them, and per root the six-point call that singles it out
    -> dict s, q1, q2 (5, 2), sol (five_point), calls [k] = dict p1, p2 (6, 2) float32, thr (px), residual (px)"""
    key = (name, seed)
    if key not in _PROBLEMS:
        s = scene(name, 5, seed)
        q1, q2 = normalise(s["p1"]), normalise(s["p2"])
        sol = five_point(q1, q2)
        calls = []
        for k, Ek in enumerate(sol["roots"]):
            a, b, res = sixth_point(Ek, seed=100 * seed + k)
            assert 2 * res <= SIXTH_THR, (name, seed, k, res)
            calls.append(dict(p1=np.concatenate([s["p1"], a[None]]), p2=np.concatenate([s["p2"], b[None]]), thr=SIXTH_THR, residual=res))
        _PROBLEMS[key] = dict(s=s, q1=q1, q2=q2, sol=sol, calls=calls)
    return _PROBLEMS[key]


def root_tolerance(sigma):
    return ROOT_MARGIN * EPS / sigma


def judge_sixth(E, prob, k):
    """a solver's E for call k of a root problem -> dict
         excused   the root (or the root the solver computed) lies under SIGMA_CUT: nothing below is asserted
         ratio     |E - E'| sigma' / 2^-52 for the certified root E' next to E of the 5-subset that explains E best (the solver may have
                   drawn any five of the six points; the sixth is rounded, so the subsets' roots differ by far more than the tolerance)
         accurate  ratio <= ROOT_MARGIN
         complete  |E - E_k| <= FIT_FACTOR (thr / F) / sigma_k: it is root k and no other
         valid     both validity measures <= VALID_FACTOR x the root tolerance"""
    call, Ek, sk = prob["calls"][k], prob["sol"]["roots"][k], prob["sol"]["sigma"][k]
    q1, q2 = normalise(call["p1"]), normalise(call["p2"])
    ratio, E2, s2, _ = nearest_root_of_subsets(E, q1, q2)
    excused = sk < SIGMA_CUT or (E2 is not None and s2 < SIGMA_CUT)
    fit = same_E(E, Ek)
    v = validity(E)
    return dict(excused=excused, ratio=ratio, accurate=ratio <= ROOT_MARGIN, fit=fit, complete=fit <= FIT_FACTOR * (call["thr"] / F) / sk,
                validity=max(v), valid=E2 is not None and max(v) <= VALID_FACTOR * root_tolerance(s2), sigma=sk)


def judge_five(E, q1, q2, roots=None):
    """a solver's E against the certified root of these five points next to it -> dict excused, ratio, accurate, valid, sampson_ok, listed
    (listed: that root is one of `roots`, the model's own solution set)"""
    Ek, sg = nearest_root(E, q1, q2)
    if Ek is None:
        # no certified root next to E: either E is no root at all, or the five points admit a family of solutions (a pure rotation fits every
        # [t]x R), which shows as a singular Jacobian at E itself and is excused like any root under the cut-off
        sg = sigma_min(E, epipolar_rows(q1, q2))
        return dict(excused=sg < SIGMA_CUT, ratio=math.inf, accurate=False, valid=False, sampson_ok=False, listed=False, sigma=sg, validity=max(validity(E)))
    tol = root_tolerance(sg)
    ratio = same_E(E, Ek) * sg / EPS
    x1 = np.concatenate([q1, np.ones((5, 1))], 1)
    x2 = np.concatenate([q2, np.ones((5, 1))], 1)
    a, b = x1 @ Ek.T, x2 @ Ek
    grad = np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2)
    d = np.abs(np.sum(x2 * (x1 @ np.asarray(E, float).T), 1)) / grad                      # normalised Sampson distance of the five points
    v = validity(E)
    return dict(excused=sg < SIGMA_CUT, ratio=ratio, accurate=ratio <= ROOT_MARGIN, validity=max(v), valid=max(v) <= VALID_FACTOR * tol,
                sampson_ok=bool(np.all(d <= (SAMPSON_ROWS * tol + 16 * EPS) / grad)), sigma=sg, root=Ek,
                listed=roots is None or any(same_E(Ek, r) <= 1e-9 for r in roots))


def judge_consensus(E, p1, p2, inliers, n_inliers, thr=1.0):
    """the returned inlier indices against the float64 mask of the returned E -> dict differs (count), outside_band (count), count_ok"""
    mask, band = consensus(E, p1, p2, thr)
    got = np.zeros(len(mask), bool)
    got[np.asarray(inliers, int)] = True
    differs = got != mask
    return dict(differs=int(differs.sum()), outside_band=int((differs & ~band).sum()), count_ok=int(n_inliers) == int(got.sum()))


def judge_pose(E, R, t, n_good, p1, p2, inliers):
    """the returned pose against LAPACK's candidates of the returned E and their counts on the returned inliers -> dict
         cand_dist   distance to the nearest candidate (<= CAND_TOL)
         counts, near  the four model counts and flagged points, `k` the candidate returned
         count_ok    |n_good - counts[k]| <= near[k] <= BAND_POINTS
         max_ok      counts[k] + near[k] >= every other count - its near"""
    q1, q2 = normalise(p1)[np.asarray(inliers, int)], normalise(p2)[np.asarray(inliers, int)]
    k, dist = which_candidate(E, R, t)
    pc = pose_counts(E, q1, q2)
    counts, near = [c[2] for c in pc], [c[3] for c in pc]
    return dict(cand_dist=dist, k=k, counts=counts, near=near, proper=max(abs(np.linalg.det(R) - 1), abs(np.linalg.norm(t) - 1)),
                count_ok=abs(int(n_good) - counts[k]) <= near[k] <= BAND_POINTS,
                max_ok=all(counts[k] + near[k] >= counts[j] - near[j] for j in range(4)) and max(near) <= BAND_POINTS)
