"""The model that defines sparse direct image alignment (vo_sparse_align, csrc/vo_align.hip): float64 numpy, written before the kernel.

The 6-DoF pose T (x_cur = R x_prev + t) of the current frame against the previous one, from the two image pyramids and n 3-D points X in the
PREVIOUS camera's coordinates: 4 x 4 patches around the projected points, photometric error, inverse-compositional Gauss-Newton, coarse to
fine.  This is the first stage of semi-direct VO (Forster, Pizzoli, Scaramuzza: "SVO: Fast Semi-Direct Monocular Visual Odometry", ICRA 2014,
section IV-A), stated here in full:

  level l   from max_level down to min_level: s = 1 / 2^l, f_l = f s, c_l = c s (the tracker's convention p_l = p / (1 << l)),
            pi_l(X) = (fx_l X.x / X.z + cx_l, fy_l X.y / X.z + cy_l)
  sample    bilinear: with x0 = floor(x), a = x - x0 (y0, b likewise): top = I00 + a (I01 - I00), bot = I10 + a (I11 - I10),
            I(x, y) = top + b (bot - top)
  interior  4 <= x < w_l - 5 and 4 <= y < h_l - 5
  reference u = pi_l(X); the row is usable when X is finite, X.z > 0 and u is in the interior; patch pixels u + o, o in {-2, -1, 0, 1}^2;
            gradient g = (0.5 (I(x + 1, y) - I(x - 1, y)), 0.5 (I(x, y + 1) - I(x, y - 1))) of the same bilinear samples of the prev level;
            J_p = dpi_l/dX [I | -[X]x] (2 x 6) of the patch CENTRE serves the 16 pixels; xi = (v, omega), translation first
  iteration Y = R X + t, v = pi_l(Y); used: usable, Y.z > 0 and v in the interior; r = I_cur(v + o) - I_prev(u + o); weight 1 where
            |r| <= huber, else huber / |r| (huber = 0: always 1); per point the 16-pixel sums G = sum w g g^T (3), e = sum w g r (2),
            q = sum w r^2; H = sum J_p^T G J_p, b = sum J_p^T e, chi = sum q / (16 n_used)
            first iteration: fewer than min_points used -> the level is skipped (iters = -1); zbar = mean Y.z of the used points
            later: fewer than min_points used, or chi > chi_prev -> the previous pose is restored and the level ends
            H xi = b by Cholesky; a pivot that is not positive ends the level with the pose kept
            T <- T E(xi)^-1 with E(xi) = (Rodrigues(omega), v): R <- R Rodrigues(omega)^T, t <- t - R v (the new R)
            max(|omega_i|, |v_i| / zbar) < eps ends the level; so does max_iters
  iters[l]  the linearisations the level evaluated (-1: skipped); n_used / used_mask / chi2: of the last linearisation whose pose was
            kept (the finest level that ran); no level ran: status VO_E_NUMERIC, pose = T0
  ends[l]   how the level ended, VO_ALIGN_END_* of include/vo_mi355x.h (0: not asked for, -1: skipped).  The tests of a linearisation come in
            this order: too few points (POINTS), chi > chi_prev (CHI; equality continues), the pivot (PIVOT), the step below eps (EPS),
            and the level's last linearisation ends it by MAX_ITERS.  flags = ends[finest level that ran] (0: no level ran)
  unused    a point that is not used still takes part in the arithmetic of its lanes: it samples at (8, 8), which on a level smaller than
            12 pixels lies in the store's 32-pixel border.  Its values never reach a sum, so the model samples a copy of the level
            padded by 32 pixels whose content does not matter (run(fill=): edge replication, or any constant)

Every stop decision returns its margin (`margins` of run()): a test can tell which runs are decided whatever the rounding.  f32=True runs the
sampling, gradient, residual and weight arithmetic and the 16-pixel sums in float32 (everything else stays float64): the yardstick for the
kernel's tolerance."""
import numpy as np

VO_E_NUMERIC = -6
END_EPS, END_MAX_ITERS, END_CHI, END_PIVOT, END_POINTS = 1, 2, 3, 4, 5                             # VO_ALIGN_END_*
END_NAMES = {0: "-", -1: "skipped", 1: "EPS", 2: "MAX_ITERS", 3: "CHI", 4: "PIVOT", 5: "POINTS"}
PAD = 32                                                                                           # the store's border
DEFAULTS = dict(max_level=-1, min_level=0, max_iters=10, min_points=10, huber=10.0, eps=1e-5)
OFFS = np.array([(ox, oy) for oy in (-2, -1, 0, 1) for ox in (-2, -1, 0, 1)], np.float64)      # pixel k of a patch: (k & 3) - 2, (k >> 2) - 2


def rodrigues(r):
    r = np.asarray(r, np.float64).reshape(3)
    th = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if th < 1e-12:
        a, b = 1.0, 0.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)
    Kx = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
    return np.eye(3) + a * Kx + b * (Kx @ Kx)


def log_so3(R):
    c = min(1.0, max(-1.0, (R[0, 0] + R[1, 1] + R[2, 2] - 1.0) / 2.0))
    th = np.arccos(c)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if th < 1e-10:
        return 0.5 * w
    return th / (2.0 * np.sin(th)) * w          # (poses near pi do not occur between consecutive frames)


def project(K, l, X):
    """pi_l of rows X (n, 3) -> (n, 2); a row with z <= 0 or a NaN gives NaN"""
    s = 1.0 / (1 << l)
    X = np.asarray(X, np.float64)
    with np.errstate(all="ignore"):
        z = np.where(X[:, 2] > 0, X[:, 2], np.nan)
        return np.stack([K[0, 0] * s * X[:, 0] / z + K[0, 2] * s, K[1, 1] * s * X[:, 1] / z + K[1, 2] * s], 1)


def interior_margin(p, w, h):
    """signed distance (pixels) of p (n, 2) to the edge of the interior: > 0 inside (NaN: -inf)"""
    with np.errstate(all="ignore"):
        m = np.minimum(np.minimum(p[:, 0] - 4.0, (w - 5.0) - p[:, 0]), np.minimum(p[:, 1] - 4.0, (h - 5.0) - p[:, 1]))
    return np.where(np.isfinite(m), m, -np.inf)


def interior(p, w, h):
    with np.errstate(all="ignore"):
        return (p[:, 0] >= 4.0) & (p[:, 0] < w - 5.0) & (p[:, 1] >= 4.0) & (p[:, 1] < h - 5.0)


def padded(img, fill=None):
    """the level with a border of PAD pixels: edge replication (fill None) or the constant `fill`"""
    return np.pad(img, PAD, mode="edge") if fill is None else np.pad(img, PAD, mode="constant", constant_values=fill)


def sample(img, x, y, ft, pad=0):
    """bilinear samples of the image at (x, y) (float64 arrays) in arithmetic of type ft; img carries a border of `pad` pixels (padded()),
    so (x, y) may lie up to pad - 1 pixels outside the level"""
    x0, y0 = np.floor(x), np.floor(y)
    a, b = (x - x0).astype(ft), (y - y0).astype(ft)
    ix, iy = x0.astype(np.int64) + pad, y0.astype(np.int64) + pad
    assert ix.size == 0 or (ix.min() >= 0 and iy.min() >= 0)    # (numpy would wrap a negative index round)
    i00, i01, i10, i11 = (img[iy, ix].astype(ft), img[iy, ix + 1].astype(ft), img[iy + 1, ix].astype(ft), img[iy + 1, ix + 1].astype(ft))
    top = i00 + a * (i01 - i00)
    bot = i10 + a * (i11 - i10)
    return top + b * (bot - top)


def jacobian(K, l, X):
    """J_p (n, 2, 6) = dpi_l/dX [I | -[X]x]"""
    s = 1.0 / (1 << l)
    fx, fy = K[0, 0] * s, K[1, 1] * s
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    iz = 1.0 / z
    A = np.zeros((len(X), 2, 3))
    A[:, 0, 0] = fx * iz; A[:, 0, 2] = -(fx * x * iz) * iz
    A[:, 1, 1] = fy * iz; A[:, 1, 2] = -(fy * y * iz) * iz
    J = np.zeros((len(X), 2, 6))
    J[:, :, :3] = A
    # -[X]x = [[0, z, -y], [-z, 0, x], [y, -x, 0]]
    x, y, z = x[:, None], y[:, None], z[:, None]
    J[:, :, 3] = A[:, :, 2] * y - A[:, :, 1] * z
    J[:, :, 4] = A[:, :, 0] * z - A[:, :, 2] * x
    J[:, :, 5] = A[:, :, 1] * x - A[:, :, 0] * y
    return J


def reference(prev, K, l, X, ft=np.float64, pad=0):
    """the reference side of a level -> dict(ok (n,), u (n, 2), I (n, 16), gx, gy (n, 16), J (n, 2, 6), margin (n,)); prev carries a border of
    `pad` pixels"""
    h, w = prev.shape[0] - 2 * pad, prev.shape[1] - 2 * pad
    X = np.asarray(X, np.float64)
    n = len(X)
    fin = np.isfinite(X).all(1) & (X[:, 2] > 0)
    u = project(K, l, np.where(fin[:, None], X, np.nan))
    ok = fin & interior(u, w, h)
    uu = np.where(ok[:, None], u, 8.0)
    px, py = uu[:, 0:1] + OFFS[None, :, 0], uu[:, 1:2] + OFFS[None, :, 1]
    I = sample(prev, px, py, ft, pad)
    gx = ft(0.5) * (sample(prev, px + 1.0, py, ft, pad) - sample(prev, px - 1.0, py, ft, pad))
    gy = ft(0.5) * (sample(prev, px, py + 1.0, ft, pad) - sample(prev, px, py - 1.0, ft, pad))
    Xs = np.where(ok[:, None], X, 1.0)
    return dict(ok=ok, u=u, I=I, gx=gx, gy=gy, J=jacobian(K, l, Xs), X=Xs, margin=interior_margin(u, w, h), n=n)


def linearise(ref, cur, K, l, R, t, huber, ft=np.float64, pad=0):
    """one linearisation at the pose (R, t) -> dict(used, n_used, H (6, 6), b (6,), chi, zsum, margin (n,), res (n, 16), w (n, 16)); cur
    carries a border of `pad` pixels"""
    h, w_ = cur.shape[0] - 2 * pad, cur.shape[1] - 2 * pad
    Y = ref["X"] @ R.T + t
    v = project(K, l, Y)
    used = ref["ok"] & (Y[:, 2] > 0) & interior(v, w_, h)
    vv = np.where(used[:, None], v, 8.0)
    px, py = vv[:, 0:1] + OFFS[None, :, 0], vv[:, 1:2] + OFFS[None, :, 1]
    r = sample(cur, px, py, ft, pad) - ref["I"]
    ar = np.abs(r)
    with np.errstate(all="ignore"):
        wt = np.where((huber > 0) & (ar > ft(huber)), ft(huber) / ar, ft(1.0)).astype(ft)
    gx, gy = ref["gx"], ref["gy"]
    wgx, wgy = wt * gx, wt * gy
    s = lambda a: a.sum(1, dtype=ft).astype(np.float64)
    gxx, gxy, gyy, ex, ey, q = s(wgx * gx), s(wgx * gy), s(wgy * gy), s(wgx * r), s(wgy * r), s((wt * r) * r)
    J0, J1 = ref["J"][:, 0], ref["J"][:, 1]
    m = used.astype(np.float64)
    H = np.einsum("n,ni,nj->ij", m * gxx, J0, J0) + np.einsum("n,ni,nj->ij", m * gxy, J0, J1) + np.einsum("n,ni,nj->ij", m * gxy, J1, J0) + \
        np.einsum("n,ni,nj->ij", m * gyy, J1, J1)
    b = (m * ex) @ J0 + (m * ey) @ J1
    n_used = int(used.sum())
    chi = float((m * q).sum() / (16.0 * n_used)) if n_used else np.inf
    return dict(used=used, n_used=n_used, H=H, b=b, chi=chi, zsum=float((m * np.where(used, Y[:, 2], 0.0)).sum()),
                margin=np.where(ref["ok"], np.minimum(interior_margin(v, w_, h), np.where(np.isfinite(Y[:, 2]), Y[:, 2], -np.inf)), np.inf), res=r, w=wt)


def cholesky_solve(H, b):
    """-> (xi, smallest pivot); xi is None where a pivot is not positive"""
    L = np.zeros((6, 6))
    piv = np.inf
    for j in range(6):
        d = H[j, j] - L[j, :j] @ L[j, :j]
        piv = min(piv, d)
        if not d > 0:
            return None, d
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (H[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x, piv


def run(prev_levels, cur_levels, K, X, rvec0=None, tvec0=None, f32=False, fill=None, **params):
    """-> dict(rvec, tvec, R, t, status, n_used, levels_run, iters [8], ends [8], flags, chi2, used (n,) bool, margins: list of
    (kind, value, threshold), points_exits: list of (level, chi, chi_prev) of the linearisations that ended a level by POINTS).  prev_levels / cur_levels: the u8 levels of the two frames, level 0 first, as the frame store holds them;
    fill: what the border that only unused points sample holds (padded())"""
    p = dict(DEFAULTS); p.update(params)
    ft = np.float32 if f32 else np.float64
    K = np.asarray(K, np.float64).reshape(3, 3)
    X = np.asarray(X, np.float32).astype(np.float64).reshape(-1, 3)
    top = len(prev_levels) - 1
    max_level = top if p["max_level"] < 0 else p["max_level"]
    assert 0 <= p["min_level"] <= max_level <= top and p["max_iters"] >= 1 and p["huber"] >= 0 and p["eps"] >= 0
    R0 = rodrigues(np.zeros(3) if rvec0 is None else rvec0)
    t0 = np.zeros(3) if tvec0 is None else np.asarray(tvec0, np.float64).reshape(3).copy()
    R, t = R0.copy(), t0.copy()
    iters, ends = np.zeros(8, np.int32), np.zeros(8, np.int32)
    margins, points_exits = [], []
    levels_run, n_used, chi2, used, flags = 0, 0, 0.0, np.zeros(len(X), bool), 0
    for l in range(max_level, p["min_level"] - 1, -1):
        prev, cur = padded(prev_levels[l], fill), padded(cur_levels[l], fill)
        ref = reference(prev, K, l, X, ft, PAD)
        margins.append(("visible_ref", np.abs(ref["margin"][np.isfinite(ref["margin"])]).min() if np.isfinite(ref["margin"]).any() else np.inf, 0.0))
        chi_prev, Rp, tp, zbar, last, end = np.inf, R, t, 1.0, None, END_MAX_ITERS
        for it in range(p["max_iters"]):
            lin = linearise(ref, cur, K, l, R, t, p["huber"], ft, PAD)
            fm = lin["margin"][np.isfinite(lin["margin"])]
            margins.append(("visible", np.abs(fm).min() if len(fm) else np.inf, 0.0))
            margins.append(("min_points", lin["n_used"], p["min_points"]))
            if it == 0:
                if lin["n_used"] < p["min_points"]:
                    iters[l], end = -1, -1
                    break
                zbar = lin["zsum"] / lin["n_used"]
            iters[l] = it + 1
            if lin["n_used"] < p["min_points"]:
                R, t, end = Rp, tp, END_POINTS
                points_exits.append((l, lin["chi"], chi_prev))          # (POINTS goes before CHI: a test wants an exit where chi rose too)
                break
            if it > 0:
                # (chi_prev = 0: chi = 0 is the tie itself, which continues; anything above it ends the level)
                margins.append(("chi", lin["chi"] / chi_prev if chi_prev > 0 else (1.0 if lin["chi"] == 0 else np.inf), 1.0))
            if lin["chi"] > chi_prev:
                R, t, end = Rp, tp, END_CHI
                break
            last = lin
            xi, piv = cholesky_solve(lin["H"], lin["b"])
            margins.append(("pivot", piv / max(np.abs(np.diag(lin["H"])).max(), 1e-300), 0.0))
            if xi is None:
                end = END_PIVOT
                break
            Rp, tp, chi_prev = R, t, lin["chi"]
            R = R @ rodrigues(xi[3:]).T
            t = t - R @ xi[:3]
            step = max(np.abs(xi[3:]).max(), np.abs(xi[:3]).max() / zbar)
            margins.append(("eps", step / p["eps"] if p["eps"] > 0 else np.inf, 1.0))
            if step < p["eps"]:
                end = END_EPS
                break
        ends[l] = end
        if iters[l] > 0:
            levels_run += 1
            n_used, chi2, used, flags = last["n_used"], last["chi"], last["used"], end
    status = 0 if levels_run else VO_E_NUMERIC
    if not levels_run:
        R, t = R0, t0
    rvec = log_so3(R) if levels_run else (np.zeros(3) if rvec0 is None else np.asarray(rvec0, np.float64).reshape(3).copy())
    return dict(rvec=rvec, tvec=t.copy(), R=R, t=t, status=status, n_used=n_used, levels_run=levels_run, iters=iters, ends=ends, flags=flags, chi2=chi2,
                used=used, margins=margins, points_exits=points_exits)


def decided(m64, m32, slack=4.0, exact=()):
    """Is every stop decision of the float64 run away from its threshold by more than `slack` x what the float32 switch moves it?  Both runs
    must have taken the same decisions in the same order; then each margin's distance to its threshold is compared with its change.
    A margin that sits ON its threshold in both runs is undecided under that rule, which is right for rounding.  exact: the kinds of margin
    a case declares to be structural zeros (a pivot that is 0 because a whole gradient component is 0, chi = chi_prev = 0 on identical
    frames, a projection that is exactly on the interior's edge): a margin of such a kind that equals its threshold in BOTH runs counts
    as decided, any other value of it falls under the general rule (exact_margins() gives the values for a test to assert)"""
    a, b = m64["margins"], m32["margins"]
    if len(a) != len(b) or any(x[0] != y[0] for x, y in zip(a, b)):
        return False
    if not (np.array_equal(m64["iters"], m32["iters"]) and np.array_equal(m64["used"], m32["used"]) and m64["n_used"] == m32["n_used"]):
        return False
    for (kind, va, thr), (_, vb, _t) in zip(a, b):
        if kind == "min_points":
            if va != vb:
                return False
            continue
        if not (np.isfinite(va) and np.isfinite(vb)):
            if va != vb and not (np.isnan(va) and np.isnan(vb)):
                return False
            continue
        if kind in exact and va == thr and vb == thr:
            continue
        if abs(va - thr) <= slack * abs(va - vb):
            return False
    return True


def exact_margins(m, kinds):
    """-> list of (kind, value, threshold) of the margins of the given kinds"""
    return [x for x in m["margins"] if x[0] in kinds]


def displacement(K, X, Ra, ta, Rb, tb):
    """largest distance (level-0 pixels) between the projections of the usable rows of X under the two poses"""
    X = np.asarray(X, np.float32).astype(np.float64).reshape(-1, 3)
    X = X[np.isfinite(X).all(1) & (X[:, 2] > 0)]
    d = project(K, 0, X @ Ra.T + ta) - project(K, 0, X @ Rb.T + tb)
    d = np.linalg.norm(d, axis=1)
    return float(np.nanmax(d)) if len(d) else 0.0


# ---- scenes ------------------------------------------------------------------------------------
def pyramid(img, levels):
    import vo_oracle as o
    out = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(levels - 1):
        out.append(o.pyr_down(out[-1]))
    return out


_SCENES = {}


def scene(w=208, h=120, n_frames=6):
    from vo_mi355x import synthetic as syn
    key = (w, h, n_frames)
    if key not in _SCENES:
        _SCENES[key] = syn.sway_scene(n_frames, w=w, h=h)
    return _SCENES[key]


def scene_points(sc, t, n, seed, margin=12):
    """n random pixels of frame t with their true 3-D points in camera t's coordinates (float32), as gt_bootstrap builds them: the frame-0
    pixel and plane depth of surface(t, uv), moved by poses[t]"""
    h, w = sc["frames"][t].shape
    rng = np.random.default_rng(seed)
    uv = np.stack([rng.uniform(margin, w - margin, n), rng.uniform(margin, h - margin, n)], 1)
    return scene_points_at(sc, t, uv)


def scene_points_at(sc, t, uv):
    """the true 3-D points, in camera t's coordinates (float32), of the pixels uv (n, 2) of frame t"""
    Z, p0 = sc["surface"](t, uv)
    K, G = sc["K"], sc["poses"][t]
    X0 = np.stack([(p0[:, 0] - K[0, 2]) / K[0, 0] * Z, (p0[:, 1] - K[1, 2]) / K[1, 1] * Z, Z], 1)
    return (X0 @ G[:3, :3].T + G[:3, 3]).astype(np.float32)


def true_pose(sc, t):
    """camera t -> camera t + 1"""
    rel = sc["poses"][t + 1] @ np.linalg.inv(sc["poses"][t])
    return rel[:3, :3], rel[:3, 3]


def prediction_error(K, X, R, t, Rt, tt):
    """(median image motion under the true pose, median distance between the projections under (R, t) and under the true pose), level-0 pixels"""
    X = np.asarray(X, np.float64)
    X = X[np.isfinite(X).all(1) & (X[:, 2] > 0)]
    p_true = project(K, 0, X @ Rt.T + tt)
    motion = np.linalg.norm(p_true - project(K, 0, X), axis=1)
    err = np.linalg.norm(project(K, 0, X @ R.T + t) - p_true, axis=1)
    return float(np.nanmedian(motion)), float(np.nanmedian(err))


# ---- the problems of tests/test_gpu_align.py (tests/test_align_model.py shows which of them the model alone decides) ----------------
W, H, LEVELS = 208, 120, 2


def aniso(K, X, k=1.25):
    """the same image points from fx != fy: fy' = k fy with y' = y / k"""
    K2 = np.array(K, np.float64); K2[1, 1] *= k
    X2 = np.array(X, np.float32); X2[:, 1] /= np.float32(k)
    return K2, X2


def gpu_cases():
    """-> list of dict(name, t (the pair is frames t, t + 1), K, X (n, 3) f32, rvec0, tvec0, params, truth: X's rows move rigidly under K)"""
    sc = scene(W, H)
    K = sc["K"]
    out = []

    def add(name, t, X, K_=K, rvec0=None, tvec0=None, truth=True, **params):
        out.append(dict(name=name, t=t, K=np.array(K_, np.float64), X=np.ascontiguousarray(X, np.float32), rvec0=rvec0, tvec0=tvec0, params=params,
                        truth=truth))
    add("n10", 0, scene_points(sc, 0, 10, 100, margin=24))
    add("n17", 1, scene_points(sc, 1, 17, 101, margin=20))
    add("n64", 2, scene_points(sc, 2, 64, 102))
    add("n200", 3, scene_points(sc, 3, 200, 103))
    Ka, Xa = aniso(K, scene_points(sc, 0, 64, 104))
    add("fx_ne_fy", 0, Xa, Ka, truth=False)
    Rt, tt = true_pose(sc, 1)
    add("init_pose", 1, scene_points(sc, 1, 64, 105), rvec0=0.5 * log_so3(Rt), tvec0=0.5 * tt)
    add("init_pose_n200", 2, scene_points(sc, 2, 200, 106), rvec0=np.array([0.002, -0.001, 0.003]), tvec0=np.array([0.05, -0.02, 0.01]))
    add("huber0", 2, scene_points(sc, 2, 64, 107), huber=0.0)
    add("huber0_n17", 3, scene_points(sc, 3, 17, 108, margin=20), huber=0.0)
    add("min_level1", 3, scene_points(sc, 3, 64, 109), min_level=1)
    # (one Gauss-Newton step per level from 6 pixels away does not arrive: compared with the model only, not with the truth)
    add("max_iters1", 0, scene_points(sc, 0, 64, 110), truth=False, max_iters=1)
    X = scene_points(sc, 1, 64, 111)
    X[3::8] = np.nan
    X[5::8, 2] *= -1.0
    X[7, 2] = 0.0
    add("nan_and_behind", 1, X)
    add("leaving", 2, scene_points(sc, 2, 128, 112, margin=5))
    add("leaving_n200", 0, scene_points(sc, 0, 200, 113, margin=6), huber=0.0)
    add("n9", 3, scene_points(sc, 3, 9, 114, margin=24), rvec0=np.array([0.001, 0.002, -0.001]), tvec0=np.array([0.01, 0.0, -0.02]), truth=False)
    return out


# ---- the edge problems of tests/test_gpu_align_edges.py: every exit, level shape and boundary (tests/test_align_model.py shows that the
# model alone decides them and which exits and shapes they reach) ----------------------------------------------------------------------
WIN4 = 3                                 # a context of window 3 keeps four levels of these small frames
K_EXACT = np.array([[128.0, 0, 64], [0, 128.0, 32], [0, 0, 1]])
K_TINY = np.array([[64.0, 0, 33], [0, 64.0, 21], [0, 0, 1]])
LOG_EXP_ANGLES = (0.5, 1.5, 2.5)
LOG_EXP_AXIS = np.array([0.02, -0.012, 1.0]) / np.linalg.norm([0.02, -0.012, 1.0])


def level_sizes(w, h, levels):
    out = [(w, h)]
    for _ in range(levels - 1):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def stripes(w=W, h=H):
    """vertical stripes: gy is exactly 0 in either arithmetic, so H[1][1] and with it the second Cholesky pivot are exactly 0"""
    return np.tile((np.arange(w) * 37 % 256).astype(np.uint8), (h, 1))


def plane_points(K, uv, z):
    """the points of depth z that project at the level-0 pixels uv (n, 2)"""
    uv = np.asarray(uv, np.float64)
    z = np.broadcast_to(np.asarray(z, np.float64), (len(uv),))
    return np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0] * z, (uv[:, 1] - K[1, 2]) / K[1, 1] * z, z], 1).astype(np.float32)


def boundary_points():
    """64 points under K_EXACT at z = 4, sixteen per level of the 208 x 120 store: X = ((u - 64) / 32, (v - 32) / 32, 4) is exact in float32
    and projects without rounding at every level.  The sixteen of level l project, in level-l pixels, on the interior's edges -- (4, 4) in,
    (3.9375, 6) out, (w_l - 5, 6) out, (w_l - 5.0625, h_l - 5.0625) in, (6, h_l - 5) out, (4, h_l - 5.0625) in -- and at ten ordinary
    interior positions (multiples of 1/16 pixel)"""
    rng = np.random.default_rng(400)
    uv = []
    for l, (w, h) in enumerate(level_sizes(W, H, 4)):
        p = [(4.0, 4.0), (3.9375, 6.0), (w - 5.0, 6.0), (w - 5.0625, h - 5.0625), (6.0, h - 5.0), (4.0, h - 5.0625)]
        p += [(6.0 + rng.integers(0, 16 * (w - 13)) / 16.0, 6.0 + rng.integers(0, 16 * (h - 13)) / 16.0) for _ in range(10)]
        uv.append(np.array(p) * (1 << l))
    X = plane_points(K_EXACT, np.concatenate(uv), 4.0)
    assert np.array_equal(project(K_EXACT, 0, X), np.concatenate(uv))
    return X


BOUNDARY_USED = (True, False, False, True, False, True)


def log_exp_r0(angle):
    return angle * LOG_EXP_AXIS


def edge_cases():
    """-> list of dict in the layout of gpu_cases() plus size (w, h), win (the context's window: it decides how many levels the store
    holds), levels, frames (prev, cur) and exact (the kinds of margin the case declares structural zeros, decided()); pose_exact: the pose
    that comes back is T0 itself; log_exp: the angle of T0's rotation, which comes back through the host's Rodrigues / log pair"""
    sc = scene(W, H)
    K = sc["K"]
    F = sc["frames"]
    out = []

    def add(name, frames, X, K_=K, rvec0=None, tvec0=None, size=(W, H), win=WIN4, levels=4, exact=(), extra=None, **params):
        out.append(dict(extra or {}, name=name, t=None, K=np.array(K_, np.float64), X=np.ascontiguousarray(X, np.float32).reshape(-1, 3), rvec0=rvec0, tvec0=tvec0,
                        params=params, truth=False, size=size, win=win, levels=levels, exact=tuple(exact),
                        frames=(np.ascontiguousarray(frames[0], np.uint8), np.ascontiguousarray(frames[1], np.uint8))))
    # four levels, even and odd sizes
    for t in range(4):
        for n in (40, 200):
            add("l4_t%d_n%d" % (t, n), (F[t], F[t + 1]), scene_points(sc, t, n, 200 + t))
    so = scene(211, 123)
    for t in range(3):
        add("odd_t%d_n100" % t, (so["frames"][t], so["frames"][t + 1]), scene_points(so, t, 100, 300 + t), so["K"], size=(211, 123))
    # levels smaller than the patch footprint: 67 x 43, 34 x 22, 17 x 11 (an interior of one row), 9 x 6 (an empty interior); the content
    # moves one pixel in x, which at fx = 64 and z = 4 is t_x = 1/16
    x0, y0 = 70, 40
    tiny = (F[0][y0:y0 + 43, x0:x0 + 67], F[0][y0:y0 + 43, x0 - 1:x0 - 1 + 67])
    rng = np.random.default_rng(500)
    Xt = plane_points(K_TINY, np.stack([rng.uniform(6, 67 - 8, 40), rng.uniform(6, 43 - 8, 40)], 1), 4.0)
    add("tiny", tiny, Xt, K_TINY, size=(67, 43))
    add("tiny_min_points1", tiny, Xt, K_TINY, size=(67, 43), min_points=1)
    # the interior's comparisons on the line: one level per call, identical frames
    Xb = boundary_points()
    for l in range(4):
        add("boundary_l%d" % l, (F[0], F[0]), Xb, K_EXACT, exact=("visible_ref", "visible"), extra=dict(pose_exact=True),
            min_level=l, max_level=l, min_points=1)
    # identical frames: the residual is exactly 0; with eps = 0 every pass is the tie chi == chi_prev == 0, which continues
    X32 = scene_points(sc, 0, 32, 600)
    add("identical", (F[0], F[0]), X32, extra=dict(pose_exact=True))
    add("identical_eps0", (F[0], F[0]), X32, exact=("chi",), extra=dict(pose_exact=True), eps=0.0)
    # a pivot that is not positive: the second one on stripes, the first one on a uniform frame
    st, un = stripes(), np.full((H, W), 77, np.uint8)
    add("stripes", (st, st), X32, exact=("pivot",), extra=dict(pose_exact=True))
    add("uniform", (un, un), X32, exact=("pivot",), extra=dict(pose_exact=True))
    # points lost while a level iterates, and a top level skipped above a level that runs (the two-level store of gpu_cases())
    by = {c["name"]: c for c in gpu_cases()}
    two = dict(win=31, levels=2)
    lv, l2 = by["leaving"], by["leaving_n200"]
    add("leaving_points", (F[2], F[3]), lv["X"], min_points=113, **two)
    add("leaving_points_min_level1", (F[2], F[3]), lv["X"], min_points=113, min_level=1, **two)
    add("leaving_top_skipped", (F[2], F[3]), lv["X"], min_points=119, **two)
    add("leaving_n200_points", (F[0], F[1]), l2["X"], min_points=178, huber=0.0, **two)
    # a level that runs above a finer one that is skipped: 32 points in a strip at the right edge of the top level's interior, all of them
    # needed; the top level's one step moves three of them past the edge of level 0 (the image moves 6 pixels to the right)
    rng = np.random.default_rng(3000)
    Xs = scene_points_at(sc, 0, np.stack([rng.uniform(190.0, 197.9, 32), rng.uniform(20, 100, 32)], 1))
    add("run_above_skipped", (F[0], F[1]), Xs, max_iters=1, min_points=32, **two)
    # the same points, top level only: its second linearisation has 8 of the 32 left AND a chi that rose.  Too few points is tested first, so
    # the level ends by POINTS (with 8 points asked for, by CHI); either way the pose that comes back is T0
    add("points_before_chi", (F[0], F[1]), Xs, extra=dict(pose_exact=True), max_iters=3, min_points=32, min_level=1, **two)
    add("chi_with_points_left", (F[0], F[1]), Xs, extra=dict(pose_exact=True), max_iters=3, min_points=8, min_level=1, **two)
    # the same exit on a level above 1: the 26 x 15 level starts on 20 points and loses one in its second linearisation
    add("l4_points_top", (F[0], F[1]), scene_points(sc, 0, 64, 2000, margin=5), min_points=20)
    # one linearisation of one level: the result is T0 E(xi)^-1, H and b of that level
    Rt, tt = true_pose(sc, 1)
    X64 = scene_points(sc, 1, 64, 700)
    for l in range(4):
        add("one_lin_l%d" % l, (F[1], F[2]), X64, rvec0=0.5 * log_so3(Rt), tvec0=0.5 * tt, min_level=l, max_level=l, max_iters=1)
    # the host's Rodrigues / log pair at large angles: the first linearisation ends by PIVOT, so the pose that comes back is T0 through
    # al_rodrigues and al_log_so3.  X = R0^T X_cur with X_cur within 40 pixels of the centre: usable in both views
    rng = np.random.default_rng(800)
    rad, phi = 40.0 * np.sqrt(rng.uniform(0, 1, 32)), rng.uniform(0, 2 * np.pi, 32)
    Xc = plane_points(K, np.stack([K[0, 2] + rad * np.cos(phi), K[1, 2] + rad * np.sin(phi)], 1), rng.uniform(4, 8, 32)).astype(np.float64)
    for a in LOG_EXP_ANGLES:
        r0 = log_exp_r0(a)
        add("log_exp_%g" % a, (st, st), Xc @ rodrigues(r0), rvec0=r0, tvec0=np.zeros(3), exact=("pivot",), extra=dict(log_exp=a), max_level=0)
    # count edges: the last of exactly 16 rounds, a round of one point, rows of NaN around one point, nothing at all
    add("count_n256", (F[3], F[4]), scene_points(sc, 3, 256, 900), size=(W, H))
    add("count_n241", (F[3], F[4]), scene_points(sc, 3, 241, 901))
    for n in (241, 256):
        X = np.full((n, 3), np.nan, np.float32)
        X[n - 1] = scene_points(sc, 3, 1, 902, margin=40)
        add("count_n%d_one_finite" % n, (F[3], F[4]), X)
    X = scene_points(sc, 3, 241, 903)
    X[:230] = np.nan
    add("count_n241_tail11", (F[3], F[4]), X)                   # eleven points, the last of them alone in the sixteenth round
    add("count_n1", (F[3], F[4]), scene_points(sc, 3, 1, 902, margin=40))
    add("count_n0", (F[3], F[4]), np.zeros((0, 3), np.float32))
    return out


def mixed_batch():
    """four sequences for ONE call on a batch = 4 context (one n, one set of parameters: min_points = 20), which leave the iteration loop
    at different points -> list of case dicts, X padded to the common n with NaN rows: a four-level problem, the stripes (PIVOT on the
    first linearisation of every level that has 20 points), nine finite rows (no level runs: VO_E_NUMERIC) and a top level that ends by
    POINTS"""
    by = {c["name"]: c for c in edge_cases()}
    nine = dict(by["l4_t1_n200"]); nine["X"] = nine["X"].copy(); nine["X"][9:] = np.nan
    stripes200 = dict(by["stripes"]); stripes200["X"] = by["l4_t2_n200"]["X"]
    seqs = [by["l4_t0_n200"], stripes200, nine, by["l4_points_top"]]
    n = max(len(c["X"]) for c in seqs)
    out = []
    for k, c in enumerate(seqs):
        c = dict(c)
        X = np.full((n, 3), np.nan, np.float32); X[:len(c["X"])] = c["X"]
        c.update(name="mixed%d_%s" % (k, c["name"]), X=X, params=dict(min_points=20))
        out.append(c)
    return out


def all_cases():
    return gpu_cases() + edge_cases()


def case_store(case):
    """-> ((w, h), win, levels) of the context a case runs on"""
    return case.get("size", (W, H)), case.get("win", 31), case.get("levels", LEVELS)


def case_frames(case):
    if "frames" in case:
        return case["frames"]
    sc = scene(W, H)
    return sc["frames"][case["t"]], sc["frames"][case["t"] + 1]


_RUNS = {}


def case_runs(case):
    """the float64 and the float32-switch run of a case, computed once -> (m64, m32)"""
    key = case["name"]
    if key not in _RUNS:
        prev, cur = case_frames(case)
        levels = case_store(case)[2]
        P, C = pyramid(prev, levels), pyramid(cur, levels)
        a = run(P, C, case["K"], case["X"], case["rvec0"], case["tvec0"], **case["params"])
        b = run(P, C, case["K"], case["X"], case["rvec0"], case["tvec0"], f32=True, **case["params"])
        _RUNS[key] = (a, b)
    return _RUNS[key]


def case_decided(case):
    a, b = case_runs(case)
    return decided(a, b, exact=case.get("exact", ()))


