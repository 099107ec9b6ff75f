"""The model that defines the recursive depth filter for track candidates (vo_depth_seed_init, vo_depth_update, csrc/vo_depth.hip): float64
numpy, written before the kernel.

Every candidate corner of a reference frame (a SEED) holds a Gaussian over the inverse distance along its bearing and a Beta over its inlier
ratio (Vogiatzis and Hernandez, "Video-based, real-time multi-view stereo", 2011); every later frame with a known pose contributes one
measurement, found by a patch search along the piece of the epipolar line the current uncertainty bounds (Forster, Pizzoli, Scaramuzza:
SVO, ICRA 2014, section V; Pizzoli et al.: REMODE, ICRA 2014).  No affine warp of the patch: the filter is for the short baselines of
consecutive frames.  Stated in full:

  seed      level-0 pixel (u, v) float32; bearing f = normalize(((u - cx) / fx, (v - cy) / fy, 1)); state mu (inverse distance along f),
            sigma2, a, b, z_range in float64; ref_id names the reference pose; flags: bit 0 converged, bit 1 diverged, bits 8.. the number
            of measurements (updates and outliers) taken; a 10 x 10 u8 patch of the reference frame centred on c = floor((u, v) + 0.5):
            patch[j][i] = I(c.x - 5 + i, c.y - 5 + j).  The inner 8 x 8 has the offsets -4..3; the border serves the gradient only.
            Creation needs 5 <= c.x <= w - 5 and 5 <= c.y <= h - 5 (the patch inside the image); otherwise ok = 0 and the seed is flagged
            diverged.  mu = 1 / depth_mean, z_range = 1 / depth_min, sigma2 = z_range^2 / 36, a = b = 10
  update    of one seed against the current frame with the pose x_cur = R x_ref + t of its ref_id, the exits in this order:
   1 SKIP_INACTIVE    a state value that is not finite, sigma2 <= 0, mu <= 0, a flag set; also a pixel (u, v) that is not finite or not
                      in [0, w) x [0, h), a ref_id outside the pose list, and a pose with an entry that is not finite or beyond 1e15 in
                      magnitude (a float64 translation that large leaves no digits for a pixel).  The state is untouched bit for bit
   2 SKIP_INVISIBLE   s = sqrt(sigma2); d_near = 1 / (mu + s), d_far = 1 / max(mu - s, 1e-8), d_mid = 1 / mu; X(d) = (R f) d + t;
                      A = pi(X(d_near)), B = pi(X(d_far)), C = pi(X(d_mid)); one of the three with not z > 0
   3 SKIP_LONG        n_steps = ceil(max(|B.x - A.x|, |B.y - A.y|)), not n_steps <= max_steps (a NaN ends here)
   4 no search        n_steps < 2: the alignment starts from floor(C + 0.5), which must be scorable (else SKIP_INVISIBLE), along the
                      derivative of pi(X(d)) by d at d_mid; a derivative of length 0 (t = 0) or not finite: SKIP_DEGENERATE
   5 the search       candidate k = 0..n_steps: the pixel floor(A + k step + 0.5), step = (B - A) / n_steps; scorable where
                      5 <= x <= w - 5 and 5 <= y <= h - 5; S = 64 sum (p - q)^2 - (sum p - sum q)^2 over the 8 x 8, an exact integer;
                      the smallest S, ties to the smallest k.  Nothing scorable: SKIP_INVISIBLE.  S_best > 64 max_score:
                      OUTLIER_NOMATCH, b += 1
   6 alignment        along dir = (B - A) / |B - A|: g = dir.x gx + dir.y gy from central differences of the patch, J = (g, 1),
                      H = [[sum g g, sum g], [sum g, 64]]; not det H > 0: OUTLIER_ALIGN.  h = 0, m = 0; an iteration: the centre
                      q = c + h dir must satisfy 4 <= q.x < w - 4, 4 <= q.y < h - 4 (else OUTLIER_ALIGN); r = (I(q + o) - patch(o)) - m with
                      the aligner's bilinear form; b = (sum g r, sum r); (dh, dm) = H^-1 b; h -= dh, m += dm; |dh| < eps_align ends it;
                      max_iters iterations without that: OUTLIER_ALIGN.  Both outliers: b += 1.  The per-pixel arithmetic and the 64-pixel
                      sums (a pairwise tree over the pixel index 8 j + i: halves of 8, 4, 2, 1, then 16, then 32) are float32 in the
                      kernel and under f32=True; everything else is float64
   7 triangulation    p = (c + h dir) + ((u, v) - floor((u, v) + 0.5)): the seed sits that far from its patch's centre;
                      f_cur = normalize(K^-1 (p, 1)); [R f, -f_cur] (d_ref, d_cur)^T = -t by its normal equations; not
                      det >= 1e-6 |t|^2 or not d_ref > 0: SKIP_DEGENERATE; z = d_ref
   8 noise            t_ref = -R^T t, a_v = f z - t_ref, alpha = acos(f . t_ref / |t_ref|), beta = acos(-a_v . t_ref / (|a_v| |t_ref|))
                      (arguments clamped to [-1, 1]), beta+ = beta + 2 atan(px_noise / (2 fx)), gamma = pi - alpha - beta+,
                      z+ = |t_ref| sin(beta+) / sin(gamma), tau = z+ - z, tau_inv = (1 / max(1e-7, z - tau) - 1 / (z + tau)) / 2
   9 Bayes            bayes() below with x = 1 / z, tau2 = tau_inv^2; a result that is not finite, or not sigma2' > 0: SKIP_DEGENERATE, the
                      state as it was.  Otherwise UPDATED
  10 flags            after every change of the state: converged when sqrt(sigma2) < z_range / conv_ratio, diverged when
                      a / (a + b) < min_inlier; the measurement count goes up by one

update(perturb=) moves A by +perturb and B by -perturb pixels in both coordinates: decided() calls a seed decided by the model alone when
perturb = +-1e-6 and the float32 switch change none of n_steps, the best k, the best pixel, the result code, the iteration count and the
flags."""
import numpy as np

UPDATED, OUTLIER_NOMATCH, OUTLIER_ALIGN, SKIP_INVISIBLE, SKIP_LONG, SKIP_DEGENERATE, SKIP_INACTIVE = range(7)     # VO_DEPTH_*
NAMES = ("UPDATED", "OUTLIER_NOMATCH", "OUTLIER_ALIGN", "SKIP_INVISIBLE", "SKIP_LONG", "SKIP_DEGENERATE", "SKIP_INACTIVE")
CONVERGED, DIVERGED, OBS_SHIFT = 1, 2, 8
POSE_MAX = 1e15
DEFAULTS = dict(max_steps=128, max_iters=10, max_score=300 * 64, eps_align=0.03, px_noise=1.0, conv_ratio=200.0, min_inlier=0.1)
SEED = np.dtype([("mu", "f8"), ("sigma2", "f8"), ("a", "f8"), ("b", "f8"), ("z_range", "f8"), ("u", "f4"), ("v", "f4"), ("ref_id", "i4"),
                 ("flags", "i4")])
assert SEED.itemsize == 56
STATE = ("mu", "sigma2", "a", "b", "z_range")


def rodrigues(r):
    from align_model import rodrigues as rod
    return rod(r)


def bearing(K, uv):
    """unit bearings (n, 3) of the level-0 pixels uv (n, 2)"""
    x, y = (uv[:, 0] - K[0, 2]) / K[0, 0], (uv[:, 1] - K[1, 2]) / K[1, 1]
    nrm = np.sqrt((x * x + y * y) + 1.0)
    return np.stack([x / nrm, y / nrm, 1.0 / nrm], 1)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def project(K, X):
    return np.stack([(K[0, 0] * X[:, 0]) / X[:, 2] + K[0, 2], (K[1, 1] * X[:, 1]) / X[:, 2] + K[1, 2]], 1)


def scorable(c, w, h):
    """can the 10 x 10 patch centred on the pixels c (n, 2) float64 be read?  (a NaN cannot)"""
    return (c[:, 0] >= 5) & (c[:, 0] <= w - 5) & (c[:, 1] >= 5) & (c[:, 1] <= h - 5)


def cut(img, cx, cy, lo, hi):
    """the patches img[cy + lo .. cy + hi) x [cx + lo .. cx + hi) of the integer centres (n,) -> (n, hi - lo, hi - lo)"""
    o = np.arange(lo, hi)
    return img[(cy[:, None] + o)[:, :, None], (cx[:, None] + o)[:, None, :]]


def init_seeds(img, uv, depth_mean, depth_min, ref_id=0):
    """-> (seeds (n,) SEED, patches (n, 100) u8, ok (n,) u8) from the reference frame img"""
    h, w = img.shape
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    n = len(uv)
    s = np.zeros(n, SEED)
    s["u"], s["v"], s["ref_id"] = uv[:, 0], uv[:, 1], ref_id
    z_range = 1.0 / float(depth_min)
    s["mu"], s["z_range"], s["sigma2"], s["a"], s["b"] = 1.0 / float(depth_mean), z_range, z_range * z_range / 36.0, 10.0, 10.0
    with np.errstate(all="ignore"):
        c = np.floor(uv.astype(np.float64) + 0.5)
        ok = scorable(c, w, h)
    ci = np.where(ok[:, None], c, 5.0).astype(np.int64)
    patches = np.where(ok[:, None], cut(img, ci[:, 0], ci[:, 1], -5, 5).reshape(n, 100), 0).astype(np.uint8)
    s["flags"] = np.where(ok, 0, DIVERGED)
    return s, patches, ok.astype(np.uint8)


def score(P, Q):
    """64 x ZMSSD of the 8 x 8 patches P, Q (.., 64) of integers, exactly"""
    P, Q = P.astype(np.int64), Q.astype(np.int64)
    d = P - Q
    return 64 * (d * d).sum(-1) - (P.sum(-1) - Q.sum(-1)) ** 2


def tree_sum(v):
    """the sum over the 64 pixels (n, 64) in the kernel's order: lanes l and l ^ 8, ^ 4, ^ 2, ^ 1 (a DPP row), then ^ 16, then ^ 32"""
    n = v.shape[0]
    v = v.reshape(n, 4, 16)
    for s in (8, 4, 2, 1):
        v = v[:, :, :s] + v[:, :, s:2 * s]
    v = v[:, :, 0]
    return (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])


def bilinear(img, x, y, ft):
    x0, y0 = np.floor(x), np.floor(y)
    a, b = (x - x0).astype(ft), (y - y0).astype(ft)
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
    i00, i01, i10, i11 = img[iy, ix].astype(ft), img[iy, ix + 1].astype(ft), img[iy + 1, ix].astype(ft), img[iy + 1, ix + 1].astype(ft)
    top = i00 + a * (i01 - i00)
    bot = i10 + a * (i11 - i10)
    return top + b * (bot - top)


def bayes(mu, sigma2, a, b, z_range, x, tau2):
    """the moment-matched Gaussian x Beta update -> (mu', sigma2', a', b')"""
    ns = np.sqrt(sigma2 + tau2)
    s2 = 1.0 / (1.0 / sigma2 + 1.0 / tau2)
    m = s2 * (mu / sigma2 + x / tau2)
    d = x - mu
    pdf = np.exp(-(d * d) / (2.0 * (ns * ns))) / (ns * np.sqrt(2.0 * np.pi))
    C1 = a / (a + b) * pdf
    C2 = b / (a + b) * (1.0 / z_range)
    nrm = C1 + C2
    C1, C2 = C1 / nrm, C2 / nrm
    f = C1 * (a + 1.0) / (a + b + 1.0) + C2 * a / (a + b + 1.0)
    e = C1 * (a + 1.0) * (a + 2.0) / ((a + b + 1.0) * (a + b + 2.0)) + C2 * a * (a + 1.0) / ((a + b + 1.0) * (a + b + 2.0))
    mu2 = C1 * m + C2 * mu
    sg2 = C1 * (s2 + m * m) + C2 * (sigma2 + mu * mu) - mu2 * mu2
    a2 = (e - f) / (f - e / f)
    b2 = a2 * (1.0 - f) / f
    return mu2, sg2, a2, b2


def triangulate(Rf, fc, t):
    """[Rf, -fc] (d_ref, d_cur)^T = -t by the normal equations -> (d_ref, det, |t|^2)"""
    aa, cc, ac = dot3(Rf, Rf), dot3(fc, fc), dot3(Rf, fc)
    at, ct = dot3(Rf, t), dot3(fc, t)
    det = aa * cc - ac * ac
    return (ac * ct - cc * at) / det, det, dot3(t, t)


def noise(f, R, t, z, px_noise, fx):
    """tau_inv of step 8"""
    t_ref = -np.stack([(R[:, 0, i] * t[:, 0] + R[:, 1, i] * t[:, 1]) + R[:, 2, i] * t[:, 2] for i in range(3)], 1)
    tn = np.sqrt(dot3(t_ref, t_ref))
    a_v = f * z[:, None] - t_ref
    an = np.sqrt(dot3(a_v, a_v))
    alpha = np.arccos(np.clip(dot3(f, t_ref) / tn, -1.0, 1.0))
    beta = np.arccos(np.clip(-dot3(a_v, t_ref) / (an * tn), -1.0, 1.0))
    beta_p = beta + 2.0 * np.arctan(px_noise / (2.0 * fx))
    gamma = (np.pi - alpha) - beta_p
    z_p = tn * np.sin(beta_p) / np.sin(gamma)
    tau = z_p - z
    return 0.5 * (1.0 / np.maximum(1e-7, z - tau) - 1.0 / (z + tau)), tau


def pose_rt(poses):
    """poses (n_ref, 6) rvec, tvec -> (R (n_ref, 3, 3), t (n_ref, 3), usable (n_ref,))"""
    poses = np.asarray(poses, np.float64).reshape(-1, 6)
    with np.errstate(all="ignore"):
        ok = np.isfinite(poses).all(1) & (np.abs(poses) <= POSE_MAX).all(1)
        R = np.stack([rodrigues(p[:3]) if o else np.eye(3) for p, o in zip(poses, ok)])
    return R, np.where(ok[:, None], poses[:, 3:], 0.0), ok


def update(seeds, patches, img, K, poses, f32=False, perturb=0.0, **params):
    """one update of every seed against the frame img -> dict(seeds (the new state), result (n,) u8, match_uv (n, 2) f64: where the seed is in the current frame, the patch's centre
    plus the seed's offset from its own patch's centre -- of the best candidate (NOMATCH) or the last alignment step; NaN where no position
    was reached, z (n,) (NaN where nothing was triangulated), n_steps, best_k, best_px (n, 2), best_S, iters (n,) (-1: none), tied (n,): a later candidate scored
    the best S too, left (n,): the alignment left the image, stats: counts of the seven codes, then of the converged and the diverged seeds, tau (n,))"""
    p = dict(DEFAULTS); p.update(params)
    ft = np.float32 if f32 else np.float64
    eps, px_noise, conv_ratio, min_inlier = (float(np.float32(p[k])) for k in ("eps_align", "px_noise", "conv_ratio", "min_inlier"))
    K = np.asarray(K, np.float64).reshape(3, 3)
    h_img, w_img = img.shape
    n = len(seeds)
    out = seeds.copy()
    res = np.full(n, -1, np.int64)
    match, zz, tau_o = np.full((n, 2), np.nan), np.full(n, np.nan), np.full(n, np.nan)
    n_steps, best_k, best_S = np.full(n, -1, np.int64), np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    best_px, iters = np.full((n, 2), -1, np.int64), np.full(n, -1, np.int64)
    Rs, ts, pose_ok = pose_rt(poses)

    def done(mask, code):
        res[mask & (res < 0)] = code

    with np.errstate(all="ignore"):
        mu, sigma2, a, b, z_range = (seeds[k].astype(np.float64) for k in STATE)
        uv = np.stack([seeds["u"], seeds["v"]], 1).astype(np.float64)
        rid = seeds["ref_id"]
        rid_ok = (rid >= 0) & (rid < len(Rs))
        ridc = np.where(rid_ok, rid, 0)
        fin = np.isfinite(mu) & np.isfinite(sigma2) & np.isfinite(a) & np.isfinite(b) & np.isfinite(z_range)
        uv_ok = (uv[:, 0] >= 0) & (uv[:, 0] < w_img) & (uv[:, 1] >= 0) & (uv[:, 1] < h_img)
        active = fin & (sigma2 > 0) & (mu > 0) & ((seeds["flags"] & 3) == 0) & uv_ok & rid_ok & pose_ok[ridc]
        done(~active, SKIP_INACTIVE)
        R, t = Rs[ridc], ts[ridc]
        f = bearing(K, uv)
        # 2
        s = np.sqrt(sigma2)
        d_near, d_far, d_mid = 1.0 / (mu + s), 1.0 / np.maximum(mu - s, 1e-8), 1.0 / mu
        Rf = np.stack([dot3(R[:, 0], f), dot3(R[:, 1], f), dot3(R[:, 2], f)], 1)
        XA, XB, XC = Rf * d_near[:, None] + t, Rf * d_far[:, None] + t, Rf * d_mid[:, None] + t
        done(~((XA[:, 2] > 0) & (XB[:, 2] > 0) & (XC[:, 2] > 0)), SKIP_INVISIBLE)
        A, B, Cc = project(K, XA) + perturb, project(K, XB) - perturb, project(K, XC)
        # 3
        D = B - A
        ns_f = np.ceil(np.maximum(np.abs(D[:, 0]), np.abs(D[:, 1])))
        done(~(ns_f <= p["max_steps"]), SKIP_LONG)
        live = res < 0
        n_steps[live] = ns_f[live].astype(np.int64)
        searching = live & (n_steps >= 2)
        # 4
        c = np.floor(Cc + 0.5)
        c_ok = scorable(c, w_img, h_img)
        nosearch = live & (n_steps < 2)
        done(nosearch & ~c_ok, SKIP_INVISIBLE)
        gd = np.stack([K[0, 0] * (Rf[:, 0] * XC[:, 2] - XC[:, 0] * Rf[:, 2]) / (XC[:, 2] * XC[:, 2]),
                       K[1, 1] * (Rf[:, 1] * XC[:, 2] - XC[:, 1] * Rf[:, 2]) / (XC[:, 2] * XC[:, 2])], 1)
        gl = np.sqrt(gd[:, 0] * gd[:, 0] + gd[:, 1] * gd[:, 1])
        done(nosearch & ~((gl > 0) & (gl < np.inf)), SKIP_DEGENERATE)
        # 5
        T10 = patches.reshape(n, 10, 10)
        T8 = T10[:, 1:9, 1:9].reshape(n, 64)
        step = D / np.where(searching, n_steps, 1)[:, None]
        bS, tied = np.full(n, np.iinfo(np.int64).max), np.zeros(n, bool)
        for k in range(int(n_steps[searching].max()) + 1 if searching.any() else 0):
            ck = np.floor((A + k * step) + 0.5)
            can = searching & (k <= n_steps) & scorable(ck, w_img, h_img)
            ci = np.where(can[:, None], ck, 5.0).astype(np.int64)
            S = score(T8, cut(img, ci[:, 0], ci[:, 1], -4, 4).reshape(n, 64))
            tied |= can & (S == bS)
            better = can & (S < bS)
            tied &= ~better
            bS[better], best_k[better] = S[better], k
            best_px[better] = ci[better]
        done(searching & (best_k < 0), SKIP_INVISIBLE)
        found = searching & (best_k >= 0)
        best_S[found] = bS[found]
        nomatch = found & (bS > 64 * int(p["max_score"]))
        off = uv - np.floor(uv + 0.5)
        match[nomatch] = best_px[nomatch] + off[nomatch]
        done(nomatch, OUTLIER_NOMATCH)
        # 6
        start = np.where(searching[:, None], best_px, np.where(c_ok[:, None], c, 5.0).astype(np.int64)).astype(np.float64)
        Dl = np.sqrt(D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1])
        dirv = np.where(searching[:, None], D / Dl[:, None], gd / gl[:, None])
        P = T10.astype(ft)
        gx = ft(0.5) * (P[:, 1:9, 2:10] - P[:, 1:9, 0:8])
        gy = ft(0.5) * (P[:, 2:10, 1:9] - P[:, 0:8, 1:9])
        g = (dirv[:, 0].astype(ft)[:, None, None] * gx + dirv[:, 1].astype(ft)[:, None, None] * gy).reshape(n, 64)
        Tf = T8.astype(ft)
        H00, H01 = tree_sum(g * g).astype(np.float64), tree_sum(g).astype(np.float64)
        det = H00 * 64.0 - H01 * H01
        done(~(det > 0), OUTLIER_ALIGN)
        hh, mm, left_o = np.zeros(n), np.zeros(n), np.zeros(n, bool)
        ox, oy = (np.arange(64) % 8 - 4).astype(np.float64), (np.arange(64) // 8 - 4).astype(np.float64)
        run = res < 0
        q = start.copy()
        for it in range(int(p["max_iters"])):
            q = np.where(run[:, None], start + hh[:, None] * dirv, q)
            inside = (q[:, 0] >= 4.0) & (q[:, 0] < w_img - 4.0) & (q[:, 1] >= 4.0) & (q[:, 1] < h_img - 4.0)
            left = run & ~inside
            left_o |= left
            match[left] = q[left] + off[left]
            done(left, OUTLIER_ALIGN)
            run = run & inside
            if not run.any():
                break
            qs = np.where(run[:, None], q, 8.0)
            smp = bilinear(img, qs[:, 0:1] + ox[None], qs[:, 1:2] + oy[None], ft)
            r = (smp - Tf) - mm.astype(ft)[:, None]
            b0, b1 = tree_sum(g * r).astype(np.float64), tree_sum(r).astype(np.float64)
            dh, dm = (64.0 * b0 - H01 * b1) / det, (H00 * b1 - H01 * b0) / det
            hh, mm = np.where(run, hh - dh, hh), np.where(run, mm + dm, mm)
            iters[run] = it + 1
            run = run & ~(np.abs(dh) < eps)
        pfin = (start + hh[:, None] * dirv) + off
        aligned = (res < 0) & ~run
        match[res < 0] = pfin[res < 0]
        done(run, OUTLIER_ALIGN)
        # 7
        fc = bearing(K, pfin)
        z, tdet, tt = triangulate(Rf, fc, t)
        tri_ok = (tdet >= 1e-6 * tt) & (z > 0)
        done(aligned & ~tri_ok, SKIP_DEGENERATE)
        # 8, 9
        tau_inv, tau = noise(f, R, t, z, px_noise, K[0, 0])
        mu2, sg2, a2, b2 = bayes(mu, sigma2, a, b, z_range, 1.0 / z, tau_inv * tau_inv)
        good = np.isfinite(mu2) & np.isfinite(sg2) & np.isfinite(a2) & np.isfinite(b2) & (sg2 > 0)
        tried = aligned & tri_ok
        zz[tried], tau_o[tried] = z[tried], tau[tried]
        done(tried & ~good, SKIP_DEGENERATE)
        done(tried & good, UPDATED)
        up = res == UPDATED
        for k, v in zip(STATE[:4], (mu2, sg2, a2, b2)):
            out[k][up] = v[up]
        outl = (res == OUTLIER_NOMATCH) | (res == OUTLIER_ALIGN)
        out["b"][outl] = b[outl] + 1.0
        # 10
        ch = up | outl
        conv = ch & (np.sqrt(out["sigma2"]) < z_range / conv_ratio)
        div = ch & (out["a"] / (out["a"] + out["b"]) < min_inlier)
        out["flags"] = np.where(ch, (seeds["flags"] + (1 << OBS_SHIFT)) | np.where(conv, CONVERGED, 0) | np.where(div, DIVERGED, 0), seeds["flags"])
    assert (res >= 0).all()
    stats = [int((res == k).sum()) for k in range(7)] + [int(((out["flags"] & CONVERGED) != 0).sum()), int(((out["flags"] & DIVERGED) != 0).sum())]
    return dict(seeds=out, result=res.astype(np.uint8), match_uv=match, z=zz, n_steps=n_steps, best_k=best_k, best_px=best_px, best_S=best_S,
                iters=iters, stats=np.array(stats, np.int32), tau=tau_o, tied=tied, left=left_o)


DISCRETE = ("result", "n_steps", "best_k", "best_px", "iters")
CONTINUOUS = ("match_uv", "z", "mu", "sigma2", "a", "b")


def continuous(run):
    """the continuous outputs of an update as one dict of (n, ...) float64 arrays"""
    d = dict(match_uv=run["match_uv"], z=run["z"])
    for k in STATE[:4]:
        d[k] = run["seeds"][k]
    return d


def same_discrete(x, y):
    """(n,) bool: the seeds whose discrete outcomes agree between two updates"""
    ok = np.ones(len(x["result"]), bool)
    for k in DISCRETE:
        ok &= (x[k] == y[k]).reshape(len(ok), -1).all(1)
    return ok & (x["seeds"]["flags"] == y["seeds"]["flags"])


# ---- scenes ------------------------------------------------------------------------------------
W, H = 208, 120
WO, HO = 131, 77
N_FRAMES = 8
_SCENES = {}


def scene(w=W, h=H):
    """the rendered sequence: two fronto-parallel textured planes (depths 10 and 6.5 in camera 0), the camera swaying sideways; frame 0
    is the reference, poses[t] is camera 0 -> camera t"""
    from vo_mi355x import synthetic as syn
    if (w, h) not in _SCENES:
        _SCENES[(w, h)] = syn.sway_scene(N_FRAMES, w=w, h=h, f=400.0 * w / 416.0 * 2.0, pose_fn=lambda t: syn.sway_pose(t, period=24.0))
    return _SCENES[(w, h)]


def pose6(Hm):
    from align_model import log_so3
    return np.concatenate([log_so3(Hm[:3, :3]), Hm[:3, 3]])


def true_mu(sc, uv):
    """the true inverse distance along the bearing of the frame-0 pixels uv"""
    Z, _ = sc["surface"](0, uv)
    return bearing(sc["K"], np.asarray(uv, np.float64))[:, 2] / Z


def on_occlusion_edge(sc, uv):
    """(n,) bool: the seed's patch covers both planes"""
    c = np.floor(np.asarray(uv, np.float64).reshape(-1, 2) + 0.5)
    Z = np.stack([sc["surface"](0, c + o)[0] for o in ((0, 0), (-5, -5), (4, -5), (-5, 4), (4, 4))])
    return Z.min(0) != Z.max(0)


def random_uv(w, h, n, seed, margin=8):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(margin, w - margin, n), rng.uniform(margin, h - margin, n)], 1).astype(np.float32)


DEPTH_MEAN, DEPTH_MIN = 8.0, 3.0


def gpu_cases():
    """-> list of dict(name, size, uv (n, 2) f32, frames: the frame indices updated against in turn (a chain carries the state), params)"""
    out = []

    def add(name, n, seed, frames, size=(W, H), margin=8, **params):
        out.append(dict(name=name, size=size, uv=random_uv(size[0], size[1], n, seed, margin), frames=tuple(frames), params=params, ref=0,
                        depth_mean=DEPTH_MEAN, depth_min=DEPTH_MIN))
    add("chain_n200", 200, 1, (1, 2, 3, 4, 5, 6))
    add("n257_edges", 257, 2, (2,), margin=2)
    add("odd_n65", 65, 3, (1, 3), size=(WO, HO), margin=3)
    add("best_pixel_n64", 64, 4, (2,), max_score=0)
    add("iters1_n63", 63, 5, (1,), max_iters=1, eps_align=0.5)
    add("steps8_n64", 64, 6, (1, 2), max_steps=8)
    add("noise_n1", 1, 7, (1, 2), px_noise=0.5, conv_ratio=50.0, min_inlier=0.45)
    return out


def case_data(case):
    """-> dict(K, ref (the reference frame), steps: list of (frame, poses (n_ref, 6)) updated against in turn, seeds, patches, ok)"""
    if "seeds" in case:
        return case
    sc = scene(*case["size"])
    seeds, patches, ok = init_seeds(sc["frames"][case["ref"]], case["uv"], case["depth_mean"], case["depth_min"])
    return dict(K=sc["K"], ref=sc["frames"][case["ref"]], steps=[(sc["frames"][t], pose6(sc["poses"][t])[None]) for t in case["frames"]],
                seeds=seeds, patches=patches, ok=ok)


# ---- the edge problems of tests/test_gpu_depth_edges.py: every exit and boundary, on a constructed pair ----------------------------
# K_E: fx = fy = 100, principal point (20, 60); the current frame shows the reference's content 50 pixels to the right, which under pose 0
# (t = (1, 0, 0), no rotation) is an inverse DEPTH of 0.5 everywhere: a seed's segment runs along its row from u + 100 (mu + s) / f.z down
# to u + 100 (mu - s) / f.z
K_E = np.array([[100.0, 0, 20.0], [0, 100.0, 60.0], [0, 0, 1]])
E_POSES = np.array([[0, 0, 0, 1.0, 0, 0],                 # 0: the sideways step
                    [0, 0, 0, 0, 0, 0],                   # 1: t = 0
                    [0, 0, 0, 0, 0, 0.5],                 # 2: along the bearing of the principal point
                    [0, 0, 0, 0, 0, -5.0],                # 3: everything behind the camera
                    [np.nan, 0, 0, 1.0, 0, 0],            # 4..7: entries that are not finite, or huge
                    [0, 0, 0, 1.0, np.inf, 0],
                    [0, 0, 0, 1e30, 0, 0],
                    [0, 1e30, 0, 1.0, 0, 0]])


def smooth_texture(w, h, seed):
    rng = np.random.default_rng(seed)
    t = rng.uniform(0, 1, (h + 16, w + 16))
    c = np.cumsum(np.cumsum(t, 0), 1)
    b = c[9:, 9:] - c[:-9, 9:] - c[9:, :-9] + c[:-9, :-9]            # 9 x 9 box sums
    b = b[:h, :w]
    return np.clip(np.round((b - b.min()) / (b.max() - b.min()) * 255.0), 0, 255).astype(np.uint8)


def edge_pair(w=W, h=H):
    tex = smooth_texture(w + 50, h, 77)
    return np.ascontiguousarray(tex[:, 50:]), np.ascontiguousarray(tex[:, :w])       # cur[y, x] = ref[y, x - 50]


def segment_seed(u, v, a_off, b_off, ref_id=0):
    """a seed row at the pixel (u, v) whose segment under pose 0 starts a_off pixels to the right of u and ends b_off to the right"""
    s = np.zeros(1, SEED)
    fz = bearing(K_E, np.array([[u, v]], np.float64))[0, 2]
    mu, sd = fz * (a_off + b_off) / 200.0, fz * (a_off - b_off) / 200.0
    s["u"], s["v"], s["ref_id"], s["mu"], s["sigma2"], s["a"], s["b"], s["z_range"] = u, v, ref_id, mu, sd * sd, 10.0, 10.0, 1.0
    return s


def edge_cases():
    """-> list of case dicts in the layout case_data() returns, plus name, size, params, labels (one per seed) and expect: label -> dict of
    what the model must say of that seed (code, n_steps, ...); tests/test_depth_model.py asserts it of the model,
    tests/test_gpu_depth_edges.py of the kernel"""
    ref, cur = edge_pair()
    out = []
    rows, labels, expect = [], [], {}

    def put(label, row, code=None, **more):
        rows.append(row); labels.append(label)
        if code is not None:
            expect[label] = dict(more, code=code)

    def good(k):
        return segment_seed(40.0 + 9 * (k % 7), 30.0 + 11 * (k % 5), 62.3, 41.7)

    # segment lengths at the principal point's row: n_steps 0 (s below the rounding of mu), 1, 2, 64, 65, max_steps, max_steps + 1
    put("steps1", segment_seed(20.0, 60.0, 50.25, 49.75), UPDATED, n_steps=1)
    put("steps2", segment_seed(20.0, 60.0, 50.75, 49.25), UPDATED, n_steps=2)
    put("steps64", segment_seed(20.0, 60.0, 81.75, 18.25), UPDATED, n_steps=64)
    put("steps65", segment_seed(20.0, 60.0, 82.25, 17.75), UPDATED, n_steps=65)
    put("steps128", segment_seed(20.0, 60.0, 133.75, 6.25), UPDATED, n_steps=128)
    put("steps129", segment_seed(20.0, 60.0, 134.25, 5.75), SKIP_LONG)
    # a segment half outside the image (the match, at u + 50 = 200, is among the candidates scored) and one wholly outside
    put("half_outside", segment_seed(150.0, 50.0, 80.3, 20.6), UPDATED)
    put("outside", segment_seed(190.0, 50.0, 80.3, 20.6), SKIP_INVISIBLE)
    # poses: t = 0, motion along the bearing, behind the camera; a pose list entry that is not usable; ref_id out of range
    put("t_zero", segment_seed(20.0, 60.0, 62.3, 41.7, 1), SKIP_DEGENERATE)
    put("along_bearing", segment_seed(20.0, 60.0, 62.3, 41.7, 2), SKIP_DEGENERATE)
    put("behind", segment_seed(60.0, 50.0, 62.3, 41.7, 3), SKIP_INVISIBLE)
    for r, nm in ((4, "pose_nan"), (5, "pose_inf"), (6, "pose_1e30_t"), (7, "pose_1e30_r"), (-1, "ref_minus1"), (8, "ref_n"), (2 ** 31 - 1, "ref_max")):
        put(nm, segment_seed(60.0, 50.0, 62.3, 41.7, r), SKIP_INACTIVE)
        put("good_after_" + nm, good(len(rows)), UPDATED)
    # seed pixels and state values that are not finite, huge or out of range; flagged seeds
    for nm, key, val in (("u_nan", "u", np.nan), ("v_inf", "v", np.inf), ("u_1e30", "u", 1e30), ("u_neg", "u", -1.0), ("mu_nan", "mu", np.nan),
                         ("mu_inf", "mu", np.inf), ("mu_1e30", "mu", 1e30), ("mu_zero", "mu", 0.0), ("mu_neg", "mu", -0.5), ("sigma2_nan", "sigma2", np.nan),
                         ("sigma2_zero", "sigma2", 0.0), ("sigma2_neg", "sigma2", -1.0), ("sigma2_inf", "sigma2", np.inf), ("a_nan", "a", np.nan),
                         ("b_inf", "b", -np.inf), ("z_range_nan", "z_range", np.nan), ("converged", "flags", CONVERGED | (3 << OBS_SHIFT)),
                         ("diverged", "flags", DIVERGED), ("both_flags", "flags", 3)):
        row = good(3); row[key] = val
        put(nm, row, SKIP_INVISIBLE if nm in ("mu_1e30",) else SKIP_INACTIVE)
        put("good_after_" + nm, good(len(rows)), UPDATED)
    # a huge but finite sigma2 or z_range is a state like any other
    row = good(5); row["sigma2"] = 1e30
    put("sigma2_1e30", row)
    seeds = np.concatenate(rows)
    main = init_seeds(ref, np.stack([seeds["u"], seeds["v"]], 1), 2.0, 1.0)
    patches = main[1].copy()
    # a flat patch on the no-search path, det H = 0: with one step, and with none at all (s is below the rounding of mu, so A == B.  With a
    # textured patch that seed's variance update is a difference of two equal numbers, whose sign is rounding noise; here it is not reached)
    flat, flat0 = segment_seed(20.0, 60.0, 50.25, 49.75), segment_seed(20.0, 60.0, 50.0, 50.0)
    flat0["sigma2"] = 1e-40
    seeds = np.concatenate([seeds, flat, flat0]); patches = np.concatenate([patches, np.full((2, 100), 77, np.uint8)])
    labels += ["flat", "steps0_flat"]
    expect["flat"], expect["steps0_flat"] = dict(code=OUTLIER_ALIGN, n_steps=1), dict(code=OUTLIER_ALIGN, n_steps=0)
    exact = ("steps0_flat", "t_zero", "along_bearing", "mu_1e30")     # A == B exactly: no perturbation leaves n_steps = 0 as it is
    base = dict(size=(W, H), K=K_E, ref=ref, steps=[(cur, E_POSES)], seeds=seeds, patches=patches, ok=np.ones(len(seeds), np.uint8), labels=labels, exact=exact)
    out.append(dict(base, name="edges", params={}, expect=expect))
    # max_steps = 64: the segment of 64 steps runs, the one of 65 is too long
    e64 = {k: dict(v) for k, v in expect.items()}
    for nm in ("steps65", "steps128"):
        e64[nm] = dict(code=SKIP_LONG)
    out.append(dict(base, name="edges_max_steps64", params=dict(max_steps=64), expect=e64))
    # S_best exactly 64 max_score, and one step of max_score below: one inner pixel of the patch moved by 8 gives S = 64 * 64 - 64 = 64 * 63
    s1 = segment_seed(70.0, 40.0, 62.3, 41.7)
    p1 = init_seeds(ref, np.array([[70.0, 40.0]]), 2.0, 1.0)[1].copy()
    k = 44 if p1[0, 44] <= 247 else 45
    p1[0, k] = p1[0, k] + 8 if p1[0, k] <= 247 else p1[0, k] - 8
    sc = dict(size=(W, H), K=K_E, ref=ref, steps=[(cur, E_POSES)], seeds=s1, patches=p1, ok=np.ones(1, np.uint8), labels=["score"])
    out.append(dict(sc, name="score_at", params=dict(max_score=63), expect=dict(score=dict(code=UPDATED, best_S=64 * 63))))
    out.append(dict(sc, name="score_above", params=dict(max_score=62), expect=dict(score=dict(code=OUTLIER_NOMATCH, best_S=64 * 63))))
    # the match at x = 205 cannot be scored; the best of the rest is the last scorable pixel, 203 (two pixels off: its score needs SVO's
    # threshold), from where the alignment leaves the image
    s3 = segment_seed(155.0, 70.0, 60.3, 40.6)
    p3 = init_seeds(ref, np.array([[155.0, 70.0]]), 2.0, 1.0)[1]
    out.append(dict(size=(W, H), K=K_E, ref=ref, steps=[(cur, E_POSES)], seeds=s3, patches=p3, ok=np.ones(1, np.uint8), labels=["leaves"],
                    name="leaves", params=dict(max_score=2000 * 64), expect=dict(leaves=dict(code=OUTLIER_ALIGN, left=True, n_steps=20))))
    # a tie: columns of period 8, so every eighth candidate scores 0; the smallest k wins
    st = np.tile((np.arange(W) % 8 * 30 + 10).astype(np.uint8), (H, 1))
    s2 = np.concatenate([segment_seed(20.0, 60.0, 81.75, 18.25), segment_seed(37.0, 33.0, 70.3, 30.6)])
    p2 = init_seeds(st, np.stack([s2["u"], s2["v"]], 1), 2.0, 1.0)[1]
    out.append(dict(size=(W, H), K=K_E, ref=st, steps=[(st, E_POSES)], seeds=s2, patches=p2, ok=np.ones(2, np.uint8), labels=["tie0", "tie1"],
                    name="tie", params={}, expect=dict(tie0=dict(code=UPDATED, best_S=0, tied=True), tie1=dict(code=UPDATED, best_S=0, tied=True))))
    return out


_RUNS = {}


def case_runs(case):
    """a case's chain under the model, computed once -> list per frame of dict(m64, m32, decided (n,) bool, seeds_in).  The float32
    switch runs a chain of its own, its state carried like the float64 one's, so its deviation accumulates the way a kernel's does; a
    seed is decided at a frame when it was at every frame before and the switch and the two perturbed updates (from the float64 state)
    leave its discrete outcomes as they are"""
    if case["name"] not in _RUNS:
        d = case_data(case)
        K, seeds, patches = d["K"], d["seeds"], d["patches"]
        seeds32, dec, steps = seeds, np.ones(len(seeds), bool), []
        for img, pose in d["steps"]:
            m64 = update(seeds, patches, img, K, pose, **case["params"])
            m32 = update(seeds32, patches, img, K, pose, f32=True, **case["params"])
            dec = dec & same_discrete(m64, m32)
            for e in (1e-6, -1e-6):
                dec = dec & same_discrete(m64, update(seeds, patches, img, K, pose, perturb=e, **case["params"]))
            steps.append(dict(m64=m64, m32=m32, decided=dec, seeds_in=seeds))
            seeds, seeds32 = m64["seeds"], m32["seeds"]
        _RUNS[case["name"]] = steps
    return _RUNS[case["name"]]
