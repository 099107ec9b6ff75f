"""numpy model of the two-view DLT triangulation (csrc/vo_dlt.hip), its test scenes and the bounds the kernel is held to.

Plain numpy, float64, no GPU and no oracle: the bounds are stated against LAPACK's SVD of the very matrix the kernel builds, so they hold for
ANY correct solver and share nothing with the Jacobi iteration of the kernel and of oracle/vo_oracle.c.

  system   A [n, 4, 4]: rows u P[2] - P[0], v P[2] - P[1] for view 0, then view 1; the float32 inputs widened to float64 first (exact), every
           product and difference in float64 like the kernel's
  svd      singular values s1 >= ... >= s4 and the last right-singular vector v4 of A

  optimality  for the returned float32 x:  |A x| / |x| <= s4 + 2 * 2^-24 * s1.  The minimum of |A x| / |x| is s4, reached at v4; rounding x to
              float32 moves it by at most 2^-24 |x|, hence the residual by at most 2^-24 s1; the factor 2 covers the float64 solver.  It holds
              for every point, rank-deficient systems included (there every vector of the null space reaches s4).
  direction   where the null vector is well separated, (s3 - s4) / s1 >= 1e-6:  sin angle(x, +-v4) <= 2^-23
  statistics  depth1, reproj as the reference computes them from the returned x (extractor.py:271, triangulate.py:15-29 of the reference): the
              float32 divide x[:3] / x[3], then float64: M = K @ H[:3], camera-1 depth from H1[2], (|e0| + |e1|) / 2.  The tolerance is per
              point: 8 x |float64 evaluation - longdouble evaluation| of this model + 16 ulp of the value; it measures the model against
              itself, never the kernel.
  filter      depth1 > 0 and reproj < max_err (k_pipe_promote, TriangulatorNL.refine) equals the model's except where the model's value lies
              within that tolerance of the threshold.
"""
import numpy as np

from vo_mi355x import synthetic as syn

K = syn.KITTI_K
U24 = 2.0 ** -24                  # unit roundoff of float32
SIN_MAX = 2.0 ** -23
GAP_MIN = 1e-6
MAX_ERR = 2.0
SEED = 2024
RVEC = (0.01, 0.03, -0.005)
SCENES = ("normal", "tiny_baseline", "pure_rotation", "identical", "far_points", "forward_epipole", "far_origin", "behind_and_wide")
DIRECTION_EXEMPT = ("identical", "far_origin")          # exempt from the direction bound only


def pose(rvec, t):
    H = np.eye(4)
    H[:3, :3], H[:3, 3] = syn.rodrigues(rvec), t
    return H


def scene(name, n=2000, seed=SEED):
    """-> dict K, H0, H1 (float64), P0, P1 (3, 4) float32, uv0, uv1 (n, 2) float32, X (n, 3) the planted points"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-15, 15, n), rng.uniform(-3, 3, n), rng.uniform(6, 80, n)], 1)
    H0, H1, noise = np.eye(4), pose(RVEC, (0.1, -0.02, -0.9)), 0.3
    if name == "normal":
        pass
    elif name == "tiny_baseline":
        H1 = pose(RVEC, (1e-3, 0.0, -1e-3))
    elif name == "pure_rotation":
        H1 = pose(RVEC, (0.0, 0.0, 0.0))
    elif name == "identical":
        H0 = H1 = pose((0.1, 0.0, 0.0), (1.0, 2.0, 3.0))
        noise = 0.0
    elif name == "far_points":
        X[:, 2] *= 1e4
    elif name == "forward_epipole":
        X[:, 0], X[:, 1] = rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n)
        H1, noise = pose((0.0, 0.0, 0.0), (0.0, 0.0, -1.0)), 0.05
    elif name == "far_origin":
        c = np.array([1500.0, -20.0, 2400.0])
        X = X + c
        for H in (H0, H1):
            H[:3, 3] = H[:3, 3] - H[:3, :3] @ c
    elif name == "behind_and_wide":
        X[:, :2] *= 6.0
        X[1::2, 2] *= -1.0
        H1 = pose((0.01, 0.4, -0.005), (2.0, -0.02, -0.9))
    else:
        raise KeyError(name)

    def proj(H):
        p = (X @ H[:3, :3].T + H[:3, 3]) @ K.T
        return (p[:, :2] / p[:, 2:3] + rng.normal(0, noise, (n, 2))).astype(np.float32)

    uv0, uv1 = proj(H0), proj(H1)
    return dict(name=name, K=K, H0=H0, H1=H1, P0=(K @ H0[:3]).astype(np.float32), P1=(K @ H1[:3]).astype(np.float32), uv0=uv0, uv1=uv1, X=X)


def args(s, stats=True):
    """the argument list of VoContext.triangulate / dlt_upload"""
    return (s["P0"], s["P1"], s["uv0"], s["uv1"]) + ((s["K"], s["H0"], s["H1"]) if stats else ())


def system(P0, P1, uv0, uv1):
    """A [n, 4, 4] float64"""
    P0, P1 = np.asarray(P0, np.float32).astype(np.float64).reshape(3, 4), np.asarray(P1, np.float32).astype(np.float64).reshape(3, 4)
    uv0, uv1 = np.asarray(uv0, np.float32).astype(np.float64).reshape(-1, 2), np.asarray(uv1, np.float32).astype(np.float64).reshape(-1, 2)
    A = np.empty((len(uv0), 4, 4))
    A[:, 0] = uv0[:, 0:1] * P0[2] - P0[0]
    A[:, 1] = uv0[:, 1:2] * P0[2] - P0[1]
    A[:, 2] = uv1[:, 0:1] * P1[2] - P1[0]
    A[:, 3] = uv1[:, 1:2] * P1[2] - P1[1]
    return A


def svd(A):
    """-> singular values [n, 4] (descending), last right-singular vector [n, 4]"""
    _, s, vh = np.linalg.svd(A)
    return s, vh[:, 3, :]


def residual_excess(A, s, X4):
    """(|A x| / |x| - s4) / (2^-24 s1) per point, x = X4[:, i] (float32, widened): the optimality bound is `<= 2`"""
    x = np.asarray(X4, np.float32).astype(np.float64).T
    with np.errstate(all="ignore"):
        r = np.linalg.norm(np.einsum("nij,nj->ni", A, x), axis=1) / np.linalg.norm(x, axis=1)
        return (r - s[:, 3]) / (U24 * s[:, 0])


def sin_angle(X4, v4):
    """sine of the angle between x and the line of v4, per point"""
    x = np.asarray(X4, np.float32).astype(np.float64).T
    with np.errstate(all="ignore"):
        x = x / np.linalg.norm(x, axis=1, keepdims=True)
        v = v4 / np.linalg.norm(v4, axis=1, keepdims=True)
        return np.linalg.norm(x - np.sum(x * v, axis=1, keepdims=True) * v, axis=1)


def gap(s):
    return (s[:, 2] - s[:, 3]) / s[:, 0]


def stats(X4, uv0, uv1, K, H0, H1, dtype=np.float64):
    """-> depth1, reproj [n] of `dtype` (float64: the model; longdouble: the evaluation that sizes the tolerance)"""
    X4 = np.asarray(X4, np.float32)
    with np.errstate(all="ignore"):
        X, Y, Z = ((X4[k] / X4[3]).astype(dtype) for k in range(3))                 # the float32 divide of the reference
        K, H0, H1 = np.asarray(K, dtype), np.asarray(H0, dtype), np.asarray(H1, dtype)
        depth1 = H1[2, 0] * X + H1[2, 1] * Y + H1[2, 2] * Z + H1[2, 3]
        e = []
        for H, uv in ((H0, uv0), (H1, uv1)):
            # M = K @ H[:3], summed in index order with one rounding per operation (numpy's matmul would hand it to whichever BLAS is
            # installed, whose order and fusion are not defined; this form is the same on every machine)
            M = K[:, 0:1] * H[0] + K[:, 1:2] * H[1] + K[:, 2:3] * H[2]
            uv =np.asarray(uv, np.float32).reshape(-1, 2).astype(dtype)
            px = M[0, 0] * X + M[0, 1] * Y + M[0, 2] * Z + M[0, 3]
            py = M[1, 0] * X + M[1, 1] * Y + M[1, 2] * Z + M[1, 3]
            pz = M[2, 0] * X + M[2, 1] * Y + M[2, 2] * Z + M[2, 3]
            du, dv = uv[:, 0] - px / pz, uv[:, 1] - py / pz
            e.append(np.sqrt(du * du + dv * dv))
        return depth1, (e[0] + e[1]) / 2


def stats_ld(X4, uv0, uv1, K, H0, H1):
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is no wider than float64 here: it cannot size the tolerance"
    return stats(X4, uv0, uv1, K, H0, H1, np.longdouble)


def stats_tol(v, v_ld):
    """per point: 8 x the spread between the two evaluations of the model + 16 ulp of the value (inf where the model is not finite)"""
    with np.errstate(all="ignore"):
        t = (8 * np.abs(v.astype(np.longdouble) - v_ld)).astype(np.float64) + 16 * np.spacing(np.abs(v))
    return np.where(np.isfinite(v) & np.isfinite(t), t, np.inf)


def model_stats(s, X4):
    """-> dict d, r (float64 model), td, tr (their tolerances) on the returned X4 of scene s"""
    d, r = stats(X4, s["uv0"], s["uv1"], s["K"], s["H0"], s["H1"])
    dl, rl = stats_ld(X4, s["uv0"], s["uv1"], s["K"], s["H0"], s["H1"])
    return dict(d=d, r=r, td=stats_tol(d, dl), tr=stats_tol(r, rl))


def stats_deviation(got, model, tol):
    """|got - model| / tol per point where the model is finite (nan for a `got` that is not finite there: it fails `<= 1`); where the model is
    not finite: 0 if `got` is not finite either, else inf"""
    fin = np.isfinite(model)
    with np.errstate(all="ignore"):
        dev = np.abs(got - model) / tol
    dev = np.where(fin & ~np.isfinite(got), np.nan, dev)
    return np.where(fin, dev, np.where(np.isfinite(got), np.inf, 0.0))


def keep(depth1, reproj, max_err=MAX_ERR):
    with np.errstate(invalid="ignore"):
        return (depth1 > 0) & (reproj < max_err)


def filter_exceptions(depth1, reproj, m, max_err=MAX_ERR):
    """-> (differs, near): points whose filter decision differs from the model's; points whose model value lies within its tolerance of a
    threshold (the only ones that may differ)"""
    differs = keep(depth1, reproj, max_err) != keep(m["d"], m["r"], max_err)
    with np.errstate(invalid="ignore"):
        near = (np.abs(m["d"]) <= m["td"]) | (np.abs(m["r"] - max_err) <= m["tr"])
    return differs, near & np.isfinite(m["d"]) & np.isfinite(m["r"])


def bits_equal(a, b):
    """same shape, type and bit patterns (NaN included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
