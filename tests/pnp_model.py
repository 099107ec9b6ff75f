"""numpy / scipy model of the 3D-2D pose stage (csrc/vo_pnp.hip: P3P RANSAC + Gauss-Newton refinement), its scenes and the bounds it is held to.

float64 / longdouble, LAPACK and scipy.optimize; no GPU.  It does not import oracle/pnp_oracle.py except for `sample4`, the documented draw
of hypothesis h (to know which four points a hypothesis was solved from).  It shares no step with Grunert's chain of the kernel and of the
oracle (A4..A0, Ferrari, u from v, e/g triads, analytic Gauss-Newton):

  P3P             the three distance equations |s_i f_i - s_j f_j|^2 = |X_i - X_j|^2 in the depths; with x = s2 / s1, y = s3 / s1 two conics
                  in (x, y), their Sylvester resultant in y by polynomial arithmetic (numpy.polymul) -> a quartic in x (Grunert's is in y),
                  roots from numpy.roots (companion eigenvalues).  Every candidate is polished by Newton on the three equations in
                  longdouble and certified by its equation residual, by the pixel residual on its own three points and by the conditioning
                  (smallest singular values of the depth Jacobian and of the three-point reprojection Jacobian).  The pose is the SVD
                  Procrustes fit (Kabsch) of the three camera points to the three world points.  Solutions are returned as a SET.
  consensus       true float64 division; a per-point flag "within the documented arithmetic of the threshold" (see BAND_*).
                  CONTRACT: there is no cheirality test -- a point behind the camera that reprojects inside the threshold counts, as with
                  cv2.projectPoints; rows holding a NaN and points with p2 == 0 never count.
  minimiser       scipy.optimize.least_squares(method="lm") at machine tolerances on (rvec, t) with the model's own projection and a
                  complex-step Jacobian; a pose is certified as the minimiser by stationarity |J^T e| / (|J| |e|).
  iteration bound log(1 - p) / log(1 - w^4), and the library's batches of 32 + 256 k.

Every tolerance below carries its derivation; the values "measured" are of the model itself or of the oracle on the CPU
(tests/test_pnp_model.py prints them), never of the kernel.
"""
import itertools
import math

import numpy as np
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation

from vo_mi355x import synthetic as syn

K0 = np.array(syn.KITTI_K, float)
EPS = 2.0 ** -52
LD = np.longdouble
W_IMG, H_IMG = 1241.0, 376.0
FIRST_BATCH, BATCH = 32, 256

# ---- certification of the model's own P3P solutions ---------------------------------------------------------------------------------------
# Newton in longdouble ends at an equation residual of a few 2^-64 relative; rounding the depths to float64 leaves 2^-53 relative in each,
# i.e. a few 2^-52 of |s|^2 in the equations.  Measured over the 7 x 400 float64 sets: 5.6e-16.  Bound = x 4, rounded up.
RES_EQ_MAX = 4e-15
# its own three points under the Kabsch pose, float64: the equation residual (a few 2^-52 relative in squared lengths) divided by the
# triangle's extent over its depth, times the focal length; a thin or a 5 cm triangle at 40 m loses 3 digits.  Measured: 2.9e-10 px worst
# (collinear kind; cluster 1.4e-10, far 1.4e-10, under 3e-11 elsewhere).  Bound = x 4.
RES_PX_MAX = 1.2e-9
IMAG_REAL = 1e-3                  # a companion eigenvalue with |imag| below this x (1 + |x|) is tried as real (a double root splits by sqrt(eps))

# ---- bounds on a P3P solver ---------------------------------------------------------------------------------------------------------------
# BACKWARD ERROR: reprojection error of a returned pose on the three points it was solved from.  The float32 pixels the library is given
# carry half an ulp = 2^-14 px = 6.1e-5 px above 1024 px (2^-15 above 512): a pose whose own three points are off by less than 1e-6 px is
# the exact solution of data moved by a sixtieth of its own rounding, whatever the conditioning.  The model reaches RES_PX_MAX, three orders less.
P3P_BACK_PX = 1e-6
# EVERY ROOT: with sigma_px the smallest singular value of the 6 x 6 Jacobian of the three reprojections with respect to (rotation, t / depth),
# a pose with backward error beta lies within beta / sigma_px of an exact solution, to first order; ROOT_MARGIN = 4 covers the second order.
# A root whose sigma_px is under SIGMA_PX_CUT (a near-double root: the first order no longer describes the error and two roots are
# closer to each other than the data's rounding moves them) is excused from "found", counted and capped.
ROOT_MARGIN = 4.0
SIGMA_PX_CUT = 1e-2               # px per unit; a well-conditioned set has sigma_px of 10 .. 1000 (F / depth x extent)
EXCUSED_MAX = 0.05

# ---- consensus ----------------------------------------------------------------------------------------------------------------------------
# The kernel divides with v_rcp_f64 + two Newton steps (pnp_rcp: "relative error ~1e-16"): u = p0 * ip2 carries at most 2 ulp, so does v.
# du = u - u_obs then carries 2^-51 |u| ABSOLUTE, and e2 = du^2 + dv^2 moves by 2 (|du| |u| + |dv| |v|) 2^-51 plus a few ulp of e2 itself:
#     |delta e2| <= BAND_ULPS x 2^-52 x (e (|u| + |v|) + e2),     e = sqrt(e2),   BAND_ULPS = 8 (4 from the above, x 2 for the products' own rounding)
# A point whose e2 is within that of thr^2 may fall on either side.  At |u| + |v| = 1600 px and thr = 2 px this is 1.4e-12 relative.
# The hypothesis pose itself is the other term: a solver within P3P_BACK_PX on its three points is within P3P_BACK_PX / sigma_px of the model's
# pose, which moves point i by |J_i| times that (J_i: its 2 x 6 reprojection Jacobian in the same coordinates); x ROOT_MARGIN.
BAND_ULPS = 8.0
BAND_POINTS = 2

# ---- minimiser ----------------------------------------------------------------------------------------------------------------------------
# The documented refinement stops when a step lowers the cost by no more than 1e-12 of it.  With c* the minimum, s = |J^T e| / (|J| |e|)
# satisfies s <= |J dx| / |e| = sqrt((c - c*) / c); a Gauss-Newton step from within the basin removes (c - c*) almost entirely, so the
# last accepted step had sqrt((c - c*) / c) <= 1e-6 BEFORE it.  STAT_TOL = 4e-6 holds for the pose after it with a margin of 4 even if the
# step gained nothing.  The model's own minimiser (LM at 1e-15) measures 1e-13 .. 1e-9.
STAT_TOL = 4e-6
# Where the residual itself is tiny (noise-free float32 data: |e| ~ 1e-5 px) the cost is only known to its own rounding: u = p0 / p2 at a
# magnitude U carries 2 eps U, the cost of n points 2 |e| x 2 eps U sqrt(2 n), and a descent that accepts only decreases ends when c - c* is
# below that: s <= sqrt(4 eps U sqrt(2 n) / |e|), with U the largest pixel coordinate; x STAT_MARGIN = 4 (the count of roundings is an
# order of magnitude: R X + t cancels world coordinates several times the depth).  The bound on s is the larger of the two.
STAT_MARGIN = 4.0


def stat_bound(uv, enorm):
    uv = np.asarray(uv, float)
    return max(STAT_TOL, STAT_MARGIN * math.sqrt(4.0 * EPS * float(np.abs(uv).max()) * math.sqrt(2.0 * len(uv)) / max(enorm, 1e-300)))
# distance to the model's minimiser: J^T J dx = J^T e gives |dx| <= |J^T e| / smin(J)^2 = s |J| |e| / smin^2 for each of the two poses -- with
# s the stationarity a pose is ALLOWED (stat_bound, not the one it happens to have) and the model's own measured one --, x MIN_MARGIN for the
# second order, plus the float64 floor of the parameters themselves 64 eps cond(J) |x|.
MIN_MARGIN = 4.0
COST_REL = 1e-9                   # as the issue states it

# ---- the planted pose, kinds ---------------------------------------------------------------------------------------------------------------
P3P_KINDS = ("general", "plane", "far", "cluster", "equilateral", "isosceles", "collinear")
EDGE_KINDS = ("rot_pi", "rot_zero", "skew", "k2", "behind")
KINDS = P3P_KINDS + EDGE_KINDS
K_SKEW = K0 + np.array([[0, 3.5, 0], [0, 0, 0], [0, 0, 0]], float)
_AXIS = np.array([0.36, -0.8, 0.48])
_POSE = dict(rot_pi=(_AXIS * (math.pi - 0.6e-5), (0.4, -0.2, 0.8)), rot_zero=(_AXIS * 0.7e-9, (0.4, -0.2, 0.8)))
_POSE_DEFAULT = ((0.11, -0.23, 0.06), (0.5, -0.3, 1.1))


def kind_K(kind):
    return K_SKEW if kind == "skew" else (2.0 * K0 if kind == "k2" else K0)


def kind_pose(kind):
    r, t = _POSE.get(kind, _POSE_DEFAULT)
    return np.array(r, float), np.array(t, float)


# =========================================================================================================================================
# geometry of the model: its own Rodrigues (complex-safe, for the complex-step Jacobian), projection
# =========================================================================================================================================
def rodrigues(r):
    r = np.asarray(r)
    th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    Kx = np.array([[0 * r[0], -r[2], r[1]], [r[2], 0 * r[0], -r[0]], [-r[1], r[0], 0 * r[0]]])
    if abs(th2) < 1e-8:                                  # series: th^6 / 5040 is below 2^-52 here
        a, b = 1.0 - th2 / 6.0 + th2 * th2 / 120.0, 0.5 - th2 / 24.0 + th2 * th2 / 720.0
    else:
        th = np.sqrt(th2)
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    return np.eye(3) + a * Kx + b * (Kx @ Kx)


def rotvec(R):
    return Rotation.from_matrix(np.asarray(R, float)).as_rotvec()


def project(K, R, t, X):
    """(n, 2) pixels, true division.  No cheirality test."""
    p = (np.asarray(X) @ np.asarray(R).T + np.asarray(t)) @ np.asarray(K).T
    with np.errstate(divide="ignore", invalid="ignore"):
        return p[:, :2] / p[:, 2:3]


def residuals(K, R, t, X, uv):
    """(n,) pixel distances"""
    d = project(K, R, t, X) - uv
    return np.sqrt((d * d).sum(1))


def _fun(x, K, X, uv):
    return (project(K, rodrigues(x[:3]), x[3:], X) - uv).ravel()


def jacobian(x, K, X, uv):
    """complex-step d residual / d (rvec, t): (2 n, 6), exact to rounding"""
    J = np.zeros((2 * len(X), 6))
    for k in range(6):
        z = np.array(x, complex)
        z[k] += 1e-30j
        J[:, k] = _fun(z, K, X, uv).imag / 1e-30
    return J


def pose_dist(r1, t1, r2, t2, scale):
    """angle of R1 R2^T and |t1 - t2| / scale, as one norm"""
    dR = rodrigues(np.asarray(r1, float)) @ rodrigues(np.asarray(r2, float)).T
    ang = math.sqrt(max(0.0, ((dR - np.eye(3)) ** 2).sum() / 2.0))       # = |sin| .. 2 |sin(a / 2)|: the angle to first order
    return math.hypot(ang, np.linalg.norm(np.asarray(t1, float) - np.asarray(t2, float)) / scale)


# =========================================================================================================================================
# P3P
# =========================================================================================================================================
def _bearings(K, uv):
    """unit bearings in longdouble: K b = (u, v, 1) by LAPACK + one step of iterative refinement in longdouble"""
    K = np.asarray(K, float)
    out = []
    for u, v in np.asarray(uv, float):
        rhs = np.array([u, v, 1.0])
        b = np.linalg.solve(K, rhs)
        r = rhs.astype(LD) - K.astype(LD) @ b.astype(LD)
        b = b.astype(LD) + np.linalg.solve(K, r.astype(float)).astype(LD)
        out.append(b / np.sqrt((b * b).sum()))
    return np.array(out, LD)


def _eqs(s, G, d2):
    """the three distance equations and their Jacobian; G = Gram matrix of the bearings, d2 = (|X1-X2|^2, |X0-X2|^2, |X0-X1|^2)"""
    pairs = ((1, 2), (0, 2), (0, 1))
    f = np.zeros(3, s.dtype)
    J = np.zeros((3, 3), s.dtype)
    for k, (i, j) in enumerate(pairs):
        f[k] = s[i] * s[i] * G[i, i] + s[j] * s[j] * G[j, j] - 2 * s[i] * s[j] * G[i, j] - d2[k]
        J[k, i] = 2 * (s[i] * G[i, i] - s[j] * G[i, j])
        J[k, j] = 2 * (s[j] * G[j, j] - s[i] * G[i, j])
    return f, J


def kabsch(Q, P):
    """R, t with Q_i ~ R P_i + t (least squares, det R = +1)"""
    Q, P = np.asarray(Q, float), np.asarray(P, float)
    qc, pc = Q.mean(0), P.mean(0)
    H = (Q - qc).T @ (P - pc)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    R = U @ D @ Vt
    return R, qc - R @ pc


def p3p(K, X3, uv3):
    """-> dict sols = [dict s, R, t, res_eq, res_px, sigma, sigma_px, zbar], uncertified = [real candidates that did not certify]"""
    X3, uv3 = np.asarray(X3, float), np.asarray(uv3, float)
    f = _bearings(K, uv3)
    G = f @ f.T
    XL = X3.astype(LD)
    d2 = np.array([((XL[1] - XL[2]) ** 2).sum(), ((XL[0] - XL[2]) ** 2).sum(), ((XL[0] - XL[1]) ** 2).sum()], LD)
    out = dict(sols=[], uncertified=[])
    if not (d2 > 0).all():
        return out
    ca, cb, cg = float(G[1, 2]), float(G[0, 2]), float(G[0, 1])
    A, C = float(d2[0] / d2[1]), float(d2[2] / d2[1])
    # (eq a) / (eq b):  x^2 + y^2 - 2 x y ca = A (1 + y^2 - 2 y cb)      (eq c) / (eq b):  1 + x^2 - 2 x cg = C (1 + y^2 - 2 y cb)
    # as quadratics in y with polynomial coefficients in x (highest power first)
    p2, p1, p0 = np.array([1.0 - A]), np.array([-2.0 * ca, 2.0 * A * cb]), np.array([1.0, 0.0, -A])
    q2, q1, q0 = np.array([-C]), np.array([2.0 * C * cb]), np.array([1.0, -2.0 * cg, 1.0 - C])
    pm, pa, ps = np.polymul, np.polyadd, np.polysub
    m20 = ps(pm(p2, q0), pm(p0, q2)); m21 = ps(pm(p2, q1), pm(p1, q2)); m10 = ps(pm(p1, q0), pm(p0, q1))
    quartic = ps(pm(m20, m20), pm(m21, m10))
    starts = []
    for x in np.roots(quartic):
        if abs(x.imag) > IMAG_REAL * (1 + abs(x)):
            continue
        for xr in {x.real, x.real + abs(x.imag), x.real - abs(x.imag)}:
            # y: both roots of the second conic and the common-root formula; Newton decides
            ys = list(np.roots([np.polyval(q2, xr), np.polyval(q1, xr), np.polyval(q0, xr)]).real)
            den = np.polyval(m21, xr)
            if den != 0:
                ys.append(-np.polyval(m20, xr) / den)
            for y in ys:
                w = 1 + y * y - 2 * y * cb
                if xr > 0 and y > 0 and w > 0:
                    s1 = math.sqrt(float(d2[1]) / w)
                    starts.append(np.array([s1, xr * s1, y * s1], LD))
    scale2 = float(d2.max())
    found = []
    for s in starts:
        for _ in range(30):
            fv, J = _eqs(s, G, d2)
            try:
                ds = np.linalg.solve(J.astype(float), -fv.astype(float)).astype(LD)
                fr = fv + J @ ds                                         # one refinement of the float64 solve
                ds = ds + np.linalg.solve(J.astype(float), -fr.astype(float)).astype(LD)
            except np.linalg.LinAlgError:
                break
            s = s + ds
            if float(np.abs(ds).max()) <= 1e-18 * float(np.abs(s).max()):
                break
        if not np.isfinite(s.astype(float)).all() or not (s > 0).all():
            continue
        s64 = s.astype(float)
        if any(np.abs(s64 - g).max() <= 1e-9 * np.abs(g).max() for g in found):
            continue
        found.append(s64)
    for s64 in found:
        fv, J = _eqs(s64.astype(LD), G, d2)
        smax = float((s64 * s64).max())
        res_eq = float(np.abs(fv).max()) / max(smax, scale2)
        Q = (s64[:, None].astype(LD) * f).astype(float)
        R, t = kabsch(Q, X3)
        res_px = float(residuals(K, R, t, X3, uv3).max())
        sv = np.linalg.svd(J.astype(float), compute_uv=False)
        zbar = float(s64.mean())
        x = np.r_[rotvec(R), t]
        J6 = jacobian(x, K, X3, uv3)
        J6[:, 3:] *= zbar
        sol = dict(s=s64, R=R, t=t, r=x[:3], res_eq=res_eq, res_px=res_px, sigma=float(sv[-1] / sv[0]),
                   sigma_px=float(np.linalg.svd(J6, compute_uv=False)[-1]), zbar=zbar)
        (out["sols"] if (res_eq <= RES_EQ_MAX and res_px <= RES_PX_MAX) else out["uncertified"]).append(sol)
    return out


def count_by_scan(K, X3, uv3, m=200001):
    """number of positive-depth P3P solutions by another count altogether: for s1 on a grid, s2 from the (0, 1) equation and s3 from the
    (0, 2) equation (two branches each), sign changes of the (1, 2) equation.  For constructed, well separated sets only."""
    f = _bearings(K, uv3).astype(float)
    G = f @ f.T
    X3 = np.asarray(X3, float)
    a2, b2, c2 = ((X3[1] - X3[2]) ** 2).sum(), ((X3[0] - X3[2]) ** 2).sum(), ((X3[0] - X3[1]) ** 2).sum()
    smax = min(math.sqrt(c2 / (1 - G[0, 1] ** 2)), math.sqrt(b2 / (1 - G[0, 2] ** 2)))
    s1 = np.linspace(0, smax, m)[1:-1]
    n = 0
    r2, r3 = np.sqrt(c2 - s1 * s1 * (1 - G[0, 1] ** 2)), np.sqrt(b2 - s1 * s1 * (1 - G[0, 2] ** 2))
    for sg2, sg3 in itertools.product((1, -1), (1, -1)):
        s2, s3 = s1 * G[0, 1] + sg2 * r2, s1 * G[0, 2] + sg3 * r3
        g = s2 * s2 + s3 * s3 - 2 * s2 * s3 * G[1, 2] - a2
        ok = (s2 > 0) & (s3 > 0)
        n += int(((g[:-1] * g[1:] < 0) & ok[:-1] & ok[1:]).sum())
    return n


# =========================================================================================================================================
# scenes: groups of four camera-frame points (the first three are the kind, the fourth is a generic extra), moved to the world by the
# planted pose
# =========================================================================================================================================
def _pix_to_cam(K, u, v, z):
    b = np.linalg.solve(np.asarray(K, float), np.array([u, v, 1.0]))
    return b / b[2] * z


def _generic(rng, K, lo=4.0, hi=40.0):
    return _pix_to_cam(K, rng.uniform(20, W_IMG - 20), rng.uniform(20, H_IMG - 20), rng.uniform(lo, hi))


def cam_group(kind, rng, K=K0, shared=None):
    """(4, 3) camera-frame points"""
    shared = shared or {}
    if kind == "plane":
        z = shared.get("z0", rng.uniform(8, 30))
        g = [_pix_to_cam(K, rng.uniform(20, W_IMG - 20), rng.uniform(20, H_IMG - 20), z) for _ in range(3)]
    elif kind == "far":
        g = [_generic(rng, K, 200, 400) for _ in range(3)]
    elif kind == "cluster":
        c = _generic(rng, K, 10, 40)
        g = [c + rng.uniform(-0.025, 0.025, 3) for _ in range(3)]
    elif kind == "equilateral":
        r, z, th = rng.uniform(1, 4), rng.uniform(8, 30), rng.uniform(0, 2 * math.pi)
        g = [np.array([r * math.cos(th + k * 2 * math.pi / 3), r * math.sin(th + k * 2 * math.pi / 3), z]) + rng.normal(0, 1e-3, 3) for k in range(3)]
    elif kind == "isosceles":                             # apex in the plane x = 0, the base mirrored in it
        x, y, z = rng.uniform(0.5, 5), rng.uniform(-1.5, 1.5), rng.uniform(6, 40)
        g = [np.array([0.0, rng.uniform(-1.5, 1.5), rng.uniform(6, 40)]), np.array([x, y, z]), np.array([-x, y, z])]
    elif kind == "collinear":
        a, b = _generic(rng, K), _generic(rng, K)
        m = a + rng.uniform(0.2, 0.8) * (b - a)
        g = [a, b, m + rng.normal(0, 1e-3, 3) * np.linalg.norm(b - a)]
    else:
        g = [_generic(rng, K) for _ in range(3)]
    extra = g[0] + rng.uniform(-0.025, 0.025, 3) if kind == "cluster" else _generic(rng, K)      # (cluster: a generic fourth point would be
    return np.array(g + [extra])                        #  extrapolated from a triangle of under a pixel over hundreds of pixels)


def to_world(Xc, r, t):
    return (np.asarray(Xc) - t) @ rodrigues(r)              # R^T (x - t), row form


_TRIPLES = {}


def triple(kind, seed, f32=False):
    """one three-point problem of a kind (+ the generic fourth): dict K, X (4, 3), uv (4, 2), r, t (planted), sol (model p3p on the first
    three).  f32: X and uv rounded to float32 as the library receives them (the planted pose is then only near a solution)"""
    key = (kind, seed, f32)
    if key not in _TRIPLES:
        rng = np.random.default_rng([P3P_KINDS.index(kind) if kind in P3P_KINDS else 7 + EDGE_KINDS.index(kind), seed])
        K = kind_K(kind)
        r, t = kind_pose(kind)
        Xc = cam_group(kind if kind in P3P_KINDS else "general", rng, K)
        X = to_world(Xc, r, t)
        if f32:
            X = X.astype(np.float32).astype(float)
        uv = project(K, rodrigues(r), t, X)
        if f32:
            uv = uv.astype(np.float32).astype(float)
        _TRIPLES[key] = dict(kind=kind, seed=seed, K=K, X=X, uv=uv, r=r, t=t, sol=p3p(K, X[:3], uv[:3]))
    return _TRIPLES[key]


def scene(kind, n, seed=1, frac_out=0.3, noise=0.3):
    """full problem: n float32 correspondences of a kind seen from the planted pose, pixel noise, gross outliers (moved by 15 +- 80 px).
    kind 'behind': a fifth of the points is mirrored through the camera centre (same pixel, negative depth)"""
    rng = np.random.default_rng([100 + KINDS.index(kind), n, seed])
    K = kind_K(kind)
    r, t = kind_pose(kind)
    shared = dict(z0=rng.uniform(8, 30))
    base = kind if kind in P3P_KINDS else "general"
    Xc = np.concatenate([cam_group(base, rng, K, shared) for _ in range((n + 3) // 4)])[:n]
    behind = np.zeros(n, bool)
    if kind == "behind":
        behind[rng.choice(n, n // 5, replace=False)] = True
        Xc[behind] *= -1.0
    X = to_world(Xc, r, t).astype(np.float32)
    uv = project(K, rodrigues(r), t, X.astype(float)) + rng.normal(0, noise, (n, 2))
    out = rng.choice(n, int(frac_out * n), replace=False)
    uv[out] += rng.uniform(-80, 80, (len(out), 2)) + 15.0
    return dict(kind=kind, n=n, K=K, X=X, uv=uv.astype(np.float32), r=r, t=t, true_inl=np.setdiff1d(np.arange(n), out), behind=behind)


# =========================================================================================================================================
# consensus, minimiser, iteration bound
# =========================================================================================================================================
def consensus(K, R, t, X, uv, thr, pose_band=None):
    """-> dict inl (bool), border (bool), e (pixel distances).  pose_band: per-point pixel band from the pose's own uncertainty (or None)"""
    X, uv = np.asarray(X, float), np.asarray(uv, float)
    p = (X @ np.asarray(R).T + t) @ np.asarray(K).T
    with np.errstate(divide="ignore", invalid="ignore"):
        pr = p[:, :2] / p[:, 2:3]
        d = pr - uv
        e2 = (d * d).sum(1)
        ok = np.isfinite(e2) & (p[:, 2] != 0)
        e = np.sqrt(np.where(ok, e2, np.inf))
        band2 = BAND_ULPS * EPS * (e * np.abs(pr).sum(1) + e2)               # on e2
        if pose_band is not None:
            band2 = band2 + 2 * e * pose_band + pose_band ** 2
        border = ok & (np.abs(e2 - thr * thr) <= band2)
    return dict(inl=ok & (e2 <= thr * thr), border=border, e=e)


def minimise(K, X, uv, idx, r0, t0):
    """the model's minimiser of the reprojection error over idx, started at (r0, t0) -> dict r, t, cost, stat, smin, J norm"""
    X, uv = np.asarray(X, float)[idx], np.asarray(uv, float)[idx]
    x0 = np.r_[np.asarray(r0, float), np.asarray(t0, float)]
    sol = least_squares(_fun, x0, jac=jacobian, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, args=(K, X, uv), max_nfev=400)
    return dict(stationarity(K, X, uv, sol.x[:3], sol.x[3:]), r=sol.x[:3], t=sol.x[3:])


def stationarity(K, X, uv, r, t):
    x = np.r_[np.asarray(r, float), np.asarray(t, float)]
    e = _fun(x, K, X, uv)
    J = jacobian(x, K, X, uv)
    sv = np.linalg.svd(J, compute_uv=False)
    ne = float(np.linalg.norm(e))
    stat = float(np.linalg.norm(J.T @ e)) / max(sv[0] * ne, 1e-300)
    return dict(cost=float(e @ e), stat=stat, smin=float(sv[-1]), jnorm=float(sv[0]), enorm=ne, xnorm=float(np.linalg.norm(x)))


def need_iters(n, n_inliers, conf):
    """log(1 - p) / log(1 - w^4): samples of four until one is all-inlier with probability p"""
    w4 = (n_inliers / n) ** 4
    if w4 >= 1.0:
        return 0.0
    if w4 <= 0.0:
        return math.inf
    return math.log(1.0 - conf) / math.log1p(-w4)


def batch_end(k):
    """smallest 32 + 256 j >= k (k >= 1)"""
    return FIRST_BATCH if k <= FIRST_BATCH else FIRST_BATCH + BATCH * int(math.ceil((k - FIRST_BATCH) / BATCH))


def hypotheses_bounds(n, n_inliers, conf=0.9999, max_iters=1000000, best=None):
    """(lo, hi) on the number of hypotheses the library reports (a multiple 32 + 256 j).  The bound is re-evaluated at the end of every batch
    from the best count so far, which never exceeds the final one: the search cannot stop before need(final) (lo, one off for the rounding
    of the bound to an integer), and it stops at the end of the batch that found `best` or at the first batch end past need(final),
    whichever is later (hi); both are capped by the batch end of max_iters.  A count equal to n gives need = 0: the batch of `best` is the last."""
    cap = batch_end(max_iters)
    need = need_iters(n, n_inliers, conf)
    lo = batch_end(max(1, need - 1)) if math.isfinite(need) else cap
    hi = batch_end(max(1, need + 1)) if math.isfinite(need) else cap
    if best is not None and best >= 0:
        hi = max(hi, batch_end(best + 1))
        lo = max(lo, batch_end(best + 1))
    else:
        hi = cap
    return min(lo, cap), min(hi, cap)


def draw(seed, h, n):
    """the documented draw of hypothesis h (oracle/pnp_oracle.py sample4): the one thing the model takes from the oracle"""
    from pnp_oracle import sample4
    return sample4(seed, h, n)


def hypothesis(K, X, uv, idx):
    """the model's own hypothesis for a draw: P3P on idx[:3], the solution with the smallest residual on idx[3] -> sol dict (+ e4) or None"""
    X, uv = np.asarray(X, float), np.asarray(uv, float)
    sols = p3p(K, X[idx[:3]], uv[idx[:3]])["sols"]
    best = None
    for s in sols:
        e4 = float(residuals(K, s["R"], s["t"], X[idx[3]:idx[3] + 1], uv[idx[3]:idx[3] + 1])[0])
        if np.isfinite(e4) and (best is None or e4 < best["e4"]):
            best = dict(s, e4=e4)
    return best


# =========================================================================================================================================
# verdicts: the same functions judge the oracle on the CPU and the kernel on the GPU
# =========================================================================================================================================
def judge_p3p(poses, prob):
    """poses: list of (R, t) a solver returned for the first three points of `prob` (a triple).  Named booleans + measured ratios:
    back_ok    every returned pose reprojects its own three points within P3P_BACK_PX
    roots_ok   every certified model solution over SIGMA_PX_CUT has a returned pose within ROOT_MARGIN x beta / sigma_px of it"""
    K, X, uv = prob["K"], prob["X"][:3], prob["uv"][:3]
    back = [float(residuals(K, R, t, X, uv).max()) for R, t in poses]
    back = [b if np.isfinite(b) else np.inf for b in back]
    worst_root, missed, excused = 0.0, [], 0
    for s in prob["sol"]["sols"]:
        if s["sigma_px"] < SIGMA_PX_CUT:
            excused += 1
            continue
        d = [pose_dist(rotvec(R), t, s["r"], s["t"], s["zbar"]) for R, t in poses]
        bound = ROOT_MARGIN * (P3P_BACK_PX + s["res_px"]) / s["sigma_px"]
        dmin = min(d) if d else np.inf
        worst_root = max(worst_root, dmin / bound)
        if dmin > bound:
            missed.append(dmin)
    return dict(back_ok=all(b <= P3P_BACK_PX for b in back), roots_ok=not missed, worst_back=max(back) if back else 0.0,
                worst_root=worst_root, missed=missed, excused=excused, n_roots=len(prob["sol"]["sols"]), n_poses=len(poses))


def judge_minimiser(res, K, X, uv, idx):
    """res: dict rvec, t, cost.  stationary: the pose is a stationary point of the reprojection error over idx; agrees: it lies within the
    conditioning-scaled bound of the model's minimiser started from it; cost_ok: its cost is the model's projection's, to COST_REL"""
    Xi, uvi = np.asarray(X, float)[idx], np.asarray(uv, float)[idx]
    if not (np.isfinite(res["rvec"]).all() and np.isfinite(res["t"]).all()):
        return dict(stationary=False, agrees=False, cost_ok=False, stat=np.inf, dist_ratio=np.inf, cost_rel=np.inf)
    own = stationarity(K, Xi, uvi, res["rvec"], res["t"])
    m = minimise(K, X, uv, idx, res["rvec"], res["t"])
    zbar = float(np.abs((Xi @ rodrigues(m["r"]).T + m["t"])[:, 2]).mean())
    dist = math.hypot(np.linalg.norm(np.asarray(res["rvec"]) - m["r"]), np.linalg.norm(np.asarray(res["t"]) - m["t"]))
    bound = MIN_MARGIN * (stat_bound(uvi, m["enorm"]) + m["stat"]) * m["jnorm"] * m["enorm"] / m["smin"] ** 2 + 64 * EPS * m["jnorm"] / m["smin"] * (1 + m["xnorm"])
    cost_rel = abs(res["cost"] - own["cost"]) / max(own["cost"], 1e-300)
    return dict(stationary=own["stat"] <= stat_bound(uvi, own["enorm"]), agrees=dist <= bound, cost_ok=cost_rel <= COST_REL, stat=own["stat"], dist_ratio=dist / bound,
                cost_rel=cost_rel, zbar=zbar, model=m)


def judge_hypotheses(st, n, conf=0.9999, max_iters=1000000):
    lo, hi = hypotheses_bounds(n, st["n_inliers"], conf, max_iters, best=st["best"])
    h = st["hypotheses"]
    return dict(multiple=h >= FIRST_BATCH and (h - FIRST_BATCH) % BATCH == 0, within=lo <= h <= hi, lo=lo, hi=hi)


def judge_winner(res, s, thr=2.0, seed=0, conf=0.9999, max_iters=1000000):
    """res: dict rvec, t, inl (indices), st (cost, n_inliers, hypotheses, best, status) of a full problem s.  The model solves draw `best`
    itself; its consensus set must equal the returned one except for flagged borderline points; the pose must be the minimiser over the set."""
    K, X, uv, n = s["K"], s["X"].astype(float), s["uv"].astype(float), s["n"]
    st = res["st"]
    out = dict(status_ok=st["status"] == 0 and st["best"] >= 0, count_ok=st["n_inliers"] == len(res["inl"]))
    if not out["status_ok"]:
        return dict(out, consensus_ok=False, stationary=False, agrees=False, cost_ok=False, hyp_ok=False)
    idx = draw(seed, st["best"], n)
    hyp = hypothesis(K, X, uv, idx)
    out["model_has_root"] = hyp is not None
    if hyp is None:
        return dict(out, consensus_ok=False, stationary=False, agrees=False, cost_ok=False, hyp_ok=False)
    # how far a solver within P3P_BACK_PX on the three points may move every other point (first order, x ROOT_MARGIN)
    x = np.r_[hyp["r"], hyp["t"]]
    Jall = jacobian(x, K, X, uv).reshape(n, 2, 6)
    Jall[:, :, 3:] *= hyp["zbar"]
    with np.errstate(invalid="ignore"):
        pose_band = ROOT_MARGIN * (P3P_BACK_PX + hyp["res_px"]) / max(hyp["sigma_px"], 1e-300) * np.nan_to_num(np.linalg.norm(Jall, axis=(1, 2)), nan=0.0)
    cs = consensus(K, hyp["R"], hyp["t"], X, uv, thr, pose_band)
    got = np.zeros(n, bool); got[res["inl"]] = True
    diff = got != cs["inl"]
    out.update(consensus_ok=bool((~diff | cs["border"]).all()) and int(diff.sum()) <= BAND_POINTS, n_diff=int(diff.sum()), n_border=int(cs["border"].sum()),
               sigma_px=hyp["sigma_px"], nan_free=not got[~np.isfinite(X).all(1) | ~np.isfinite(uv).all(1)].any())
    jm = judge_minimiser(dict(rvec=res["rvec"], t=res["t"], cost=st["cost"]), K, X, uv, np.asarray(res["inl"]))
    jh = judge_hypotheses(st, n, conf, max_iters)
    out.update(stationary=jm["stationary"], agrees=jm["agrees"], cost_ok=jm["cost_ok"], hyp_ok=jh["multiple"] and jh["within"],
               stat=jm["stat"], dist_ratio=jm["dist_ratio"], cost_rel=jm["cost_rel"], lo=jh["lo"], hi=jh["hi"])
    return out


WINNER_KEYS = ("status_ok", "count_ok", "consensus_ok", "stationary", "agrees", "cost_ok", "hyp_ok")


# ---- (a) every root through a fourth correspondence ----------------------------------------------------------------------------------------
FOURTH_SETS = 32                  # three-point sets per kind
FOURTH_MARGIN = 4.0
FOURTH_SEED = 7                   # the search seed of the n = 4 calls
# The float32 data floor: half an ulp of a pixel above 1024 px is 2^-14 = 6.1e-5 px, the rounding of X (2^-24 relative) projects to as much;
# a pose solved from three such points extrapolates that to the fourth by |J_4| / sigma_px.  Sets whose model hypotheses -- all four draws, every
# solution -- stay under 100 x the floor are taken (in seed order, the first FOURTH_SETS of each kind): the threshold of the batch is then
# under 4 x 1e-2 px, tight against the 0.24 .. 7.5 px the unpolished solver was off by.  The choice is the model's alone.
FOURTH_FLOOR_MAX = 1e-2
# and whose hypotheses all lie over SIGMA_PX_CUT, the model's one conditioning cut, so that every one of them is a "must".
# What the solver still loses among these calls is NAMED, not selected away: FOURTH_KNOWN_MISSES lists (seed, k) of the calls whose root
# the refined solver does not reach from hypothesis 0 (found on the CPU oracle by tests/test_pnp_model.py, which prints the nearest
# distance); the CPU file asserts that exactly these calls fail, the GPU file that no other call does (check_fourth), on `best_ok` alone,
# and that every other call passes every verdict.
#   cluster    Grunert's coefficients are differences of cosines within 1e-6 of 1 for a triangle of under a pixel: the quartic loses its roots
#   collinear  next to a double root (sigma_px 0.016) Newton from either quartic root lands on the same neighbour; the other root is lost
FOURTH_KNOWN_MISSES = dict(cluster=((5, 0), (5, 1), (9, 0), (9, 1), (18, 0), (18, 1), (23, 0), (23, 1), (30, 0), (30, 1)), collinear=((18, 1),))
_FOURTH = {}


def _fourth_set(kind, seed):
    """the calls of one float32 three-point set: one per certified model solution k, or None if the model does not vouch for every draw"""
    p = triple(kind, seed, f32=True)
    calls = []
    for k, s in enumerate(p["sol"]["sols"]):
        X = p["X"].copy()
        uv = p["uv"].copy()
        uv[3] = project(p["K"], s["R"], s["t"], X[3:4])[0].astype(np.float32)
        per = {}
        for j in range(4):
            h = hypothesis(p["K"], X, uv, [i for i in range(4) if i != j] + [j])
            if h is None or h["sigma_px"] < SIGMA_PX_CUT:
                return None
            h["e_max"] = float(residuals(p["K"], h["R"], h["t"], X, uv).max())
            if not h["e_max"] <= FOURTH_FLOOR_MAX:
                return None
            per[j] = h
        calls.append(dict(kind=kind, seed=seed, k=k, K=p["K"], X=X.astype(np.float32), uv=uv.astype(np.float32), per=per, sol=s))
    return calls or None


def fourth_calls(kind):
    """-> dict calls = [dict K, X (4, 3) f32, uv (4, 2) f32, k, seed, per = {fourth index: model hypothesis with e_max}], thr, seeds.
    For every float32 three-point set of the kind and every certified model solution k, the fourth point is observed under pose k and
    rounded to float32.  The model solves each of the four draws (which point is the fourth) itself; thr = FOURTH_MARGIN x the largest
    four-point residual of its hypotheses over all draws of the batch: the float32 data floor times the extrapolation from three points to
    the fourth, nothing chosen."""
    if kind not in _FOURTH:
        calls, seeds = [], []
        for seed in range(40 * FOURTH_SETS):
            c = _fourth_set(kind, seed)
            if c is not None:
                calls += c
                seeds.append(seed)
            if len(seeds) == FOURTH_SETS:
                break
        thr = FOURTH_MARGIN * max(h["e_max"] for c in calls for h in c["per"].values())
        _FOURTH[kind] = dict(calls=calls, thr=thr, seeds=seeds)
    return _FOURTH[kind]


def judge_fourth(res, call, thr):
    """res: dict rvec, t, inl, st of one n = 4 call.  must: hypotheses h < 32 the model says reach four (its residual under thr / 4);
    must_not: over 4 thr.  Hypotheses between the marks, or solved from a draw whose root is under SIGMA_PX_CUT, excuse the call."""
    st = res["st"]
    must, must_not = [], []
    for h in range(FIRST_BATCH):
        m = call["per"][draw(FOURTH_SEED, h, 4)[3]]
        if m is not None and m["sigma_px"] >= SIGMA_PX_CUT and m["e_max"] < thr / 4:
            must.append(h)
        elif m is None or (m["e_max"] > 4 * thr and m["sigma_px"] >= SIGMA_PX_CUT):
            must_not.append(h)
    out = dict(status_ok=st["status"] == 0, four=st["n_inliers"] == 4 and len(res["inl"]) == 4, hyps_ok=st["hypotheses"] == FIRST_BATCH,
               finite=bool(np.isfinite(res["rvec"]).all() and np.isfinite(res["t"]).all()))
    excused = not must or (0 <= st["best"] < must[0] and st["best"] not in must_not)
    out["excused"] = bool(excused)
    out["best_ok"] = bool(excused or st["best"] == must[0])
    out["not_forbidden"] = st["best"] not in must_not
    jm = judge_minimiser(dict(rvec=res["rvec"], t=res["t"], cost=st["cost"]), call["K"], call["X"].astype(float), call["uv"].astype(float), np.arange(4))
    out.update(stationary=jm["stationary"], agrees=jm["agrees"], stat=jm["stat"], dist_ratio=jm["dist_ratio"])
    return out


FOURTH_KEYS = ("status_ok", "four", "hyps_ok", "finite", "best_ok", "not_forbidden", "stationary", "agrees")


def fourth_verdicts(kind, results):
    """judge_fourth on every call of a kind -> dict excused, stat, dist_ratio (worst), failing = {(seed, k): [verdicts that are False]};
    asserts nothing.  check_fourth holds `failing` against FOURTH_KNOWN_MISSES."""
    fc = fourth_calls(kind)
    out = dict(excused=0, stat=0.0, dist_ratio=0.0, failing={}, n=len(fc["calls"]), thr=fc["thr"])
    for c, r in zip(fc["calls"], results):
        j = judge_fourth(r, c, fc["thr"])
        out["excused"] += j["excused"]
        out["stat"], out["dist_ratio"] = max(out["stat"], j["stat"]), max(out["dist_ratio"], j["dist_ratio"])
        bad = [k for k in FOURTH_KEYS if not j[k]]
        if bad:
            out["failing"][(c["seed"], c["k"])] = bad
    return out


def check_fourth(kind, v, exact):
    """the verdict of part (a) for a kind: every call passes every verdict, except that the documented misses may fail, on `best_ok` alone
    (a later hypothesis, solved from another triple, still reaches the four points: status, count, pose and minimiser hold for them too).
    exact (the oracle, on the CPU): exactly the documented calls fail.  Not exact (the kernel): no other call fails -- these roots sit where
    rounding decides whether the quartic's double root comes out real, and the kernel's fused and library arithmetic differs from numpy's in
    the last place, so it reaches some of them (measured on the MI355X: 2 of the 5 cluster sets missed, the collinear call found)."""
    known = set(FOURTH_KNOWN_MISSES.get(kind, ()))
    assert v["excused"] <= EXCUSED_MAX * v["n"], v["excused"]
    assert (set(v["failing"]) == known) if exact else (set(v["failing"]) <= known), (kind, "failing calls", sorted(v["failing"].items()), "documented", sorted(known))
    assert all(bad == ["best_ok"] for bad in v["failing"].values()), v["failing"]


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, float), np.ascontiguousarray(b, float)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
