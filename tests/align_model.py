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

Every stop decision returns its margin (`margins` of run()): a test can tell which runs are decided whatever the rounding.  f32=True runs the
sampling, gradient, residual and weight arithmetic and the 16-pixel sums in float32 (everything else stays float64): the yardstick for the
kernel's tolerance."""
import numpy as np

VO_E_NUMERIC = -6
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


def sample(img, x, y, ft):
    """bilinear samples of the u8 image at (x, y) (float64 arrays inside the image) in arithmetic of type ft"""
    x0, y0 = np.floor(x), np.floor(y)
    a, b = (x - x0).astype(ft), (y - y0).astype(ft)
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
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


def reference(prev, K, l, X, ft=np.float64):
    """the reference side of a level -> dict(ok (n,), u (n, 2), I (n, 16), gx, gy (n, 16), J (n, 2, 6), margin (n,))"""
    h, w = prev.shape
    X = np.asarray(X, np.float64)
    n = len(X)
    fin = np.isfinite(X).all(1) & (X[:, 2] > 0)
    u = project(K, l, np.where(fin[:, None], X, np.nan))
    ok = fin & interior(u, w, h)
    uu = np.where(ok[:, None], u, 8.0)
    px, py = uu[:, 0:1] + OFFS[None, :, 0], uu[:, 1:2] + OFFS[None, :, 1]
    I = sample(prev, px, py, ft)
    gx = ft(0.5) * (sample(prev, px + 1.0, py, ft) - sample(prev, px - 1.0, py, ft))
    gy = ft(0.5) * (sample(prev, px, py + 1.0, ft) - sample(prev, px, py - 1.0, ft))
    Xs = np.where(ok[:, None], X, 1.0)
    return dict(ok=ok, u=u, I=I, gx=gx, gy=gy, J=jacobian(K, l, Xs), X=Xs, margin=interior_margin(u, w, h), n=n)


def linearise(ref, cur, K, l, R, t, huber, ft=np.float64):
    """one linearisation at the pose (R, t) -> dict(used, n_used, H (6, 6), b (6,), chi, zsum, margin (n,), res (n, 16), w (n, 16))"""
    h, w_ = cur.shape
    Y = ref["X"] @ R.T + t
    v = project(K, l, Y)
    used = ref["ok"] & (Y[:, 2] > 0) & interior(v, w_, h)
    vv = np.where(used[:, None], v, 8.0)
    px, py = vv[:, 0:1] + OFFS[None, :, 0], vv[:, 1:2] + OFFS[None, :, 1]
    r = sample(cur, px, py, ft) - ref["I"]
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


def run(prev_levels, cur_levels, K, X, rvec0=None, tvec0=None, f32=False, **params):
    """-> dict(rvec, tvec, R, t, status, n_used, levels_run, iters [8], chi2, used (n,) bool, margins: list of (kind, value, threshold)).
    prev_levels / cur_levels: the u8 levels of the two frames, level 0 first, as the frame store holds them"""
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
    iters = np.zeros(8, np.int32)
    margins = []
    levels_run, n_used, chi2, used = 0, 0, 0.0, np.zeros(len(X), bool)
    for l in range(max_level, p["min_level"] - 1, -1):
        ref = reference(prev_levels[l], K, l, X, ft)
        margins.append(("visible_ref", np.abs(ref["margin"][np.isfinite(ref["margin"])]).min() if np.isfinite(ref["margin"]).any() else np.inf, 0.0))
        chi_prev, Rp, tp, zbar, last = np.inf, R, t, 1.0, None
        for it in range(p["max_iters"]):
            lin = linearise(ref, cur_levels[l], K, l, R, t, p["huber"], ft)
            fm = lin["margin"][np.isfinite(lin["margin"])]
            margins.append(("visible", np.abs(fm).min() if len(fm) else np.inf, 0.0))
            margins.append(("min_points", lin["n_used"], p["min_points"]))
            if it == 0:
                if lin["n_used"] < p["min_points"]:
                    iters[l] = -1
                    break
                zbar = lin["zsum"] / lin["n_used"]
            iters[l] = it + 1
            if lin["n_used"] < p["min_points"]:
                R, t = Rp, tp
                break
            if it > 0:
                margins.append(("chi", lin["chi"] / chi_prev if chi_prev > 0 else np.inf, 1.0))
            if lin["chi"] > chi_prev:
                R, t = Rp, tp
                break
            last = lin
            xi, piv = cholesky_solve(lin["H"], lin["b"])
            margins.append(("pivot", piv / max(np.abs(np.diag(lin["H"])).max(), 1e-300), 0.0))
            if xi is None:
                break
            Rp, tp, chi_prev = R, t, lin["chi"]
            R = R @ rodrigues(xi[3:]).T
            t = t - R @ xi[:3]
            step = max(np.abs(xi[3:]).max(), np.abs(xi[:3]).max() / zbar)
            margins.append(("eps", step / p["eps"] if p["eps"] > 0 else np.inf, 1.0))
            if step < p["eps"]:
                break
        if iters[l] > 0:
            levels_run += 1
            n_used, chi2, used = last["n_used"], last["chi"], last["used"]
    status = 0 if levels_run else VO_E_NUMERIC
    if not levels_run:
        R, t = R0, t0
    rvec = log_so3(R) if levels_run else (np.zeros(3) if rvec0 is None else np.asarray(rvec0, np.float64).reshape(3).copy())
    return dict(rvec=rvec, tvec=t.copy(), R=R, t=t, status=status, n_used=n_used, levels_run=levels_run, iters=iters, chi2=chi2, used=used,
                margins=margins)


def decided(m64, m32, slack=4.0):
    """Is every stop decision of the float64 run away from its threshold by more than `slack` x what the float32 switch moves it?  Both runs
    must have taken the same decisions in the same order; then each margin's distance to its threshold is compared with its change"""
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
        if abs(va - thr) <= slack * abs(va - vb):
            return False
    return True


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


_RUNS = {}


def case_runs(case):
    """the float64 and the float32-switch run of a case, computed once -> (m64, m32)"""
    key = case["name"]
    if key not in _RUNS:
        sc = scene(W, H)
        P, C = pyramid(sc["frames"][case["t"]], LEVELS), pyramid(sc["frames"][case["t"] + 1], LEVELS)
        a = run(P, C, case["K"], case["X"], case["rvec0"], case["tvec0"], **case["params"])
        b = run(P, C, case["K"], case["X"], case["rvec0"], case["tvec0"], f32=True, **case["params"])
        _RUNS[key] = (a, b)
    return _RUNS[key]
