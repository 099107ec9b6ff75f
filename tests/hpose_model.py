"""numpy model of the pose from a homography (csrc/vo_hpose.hip: cv2.decomposeHomographyMat with counted visibility votes, a ranking and an
ambiguity verdict), a 60-digit mpmath restatement of the decomposition with its sensitivity, the exact scenes, and the bound the library is
held to.  Plain numpy float64 and mpmath; no GPU.

Decomposition   G = K^-1 H K (K read as fx, fy, cx, cy), negated if det G < 0 (both cameras on the same side of the plane: a property of H
                alone); det G = 0, a zero focal length or an entry that is not finite has no solution (VO_E_NUMERIC, NaN outputs).
                G V = U S by one-sided Jacobi rotations of the columns (the condition of G is never squared), s1 >= s2 >= s3, v3 = v1 x v2,
                u3 = u1 x u2 (both proper, as det G > 0).  With a = (s1 - s2) / s2, b = (s2 - s3) / s2, w = (s1 - s3) / s2 and
                r1 = s1 / s2, r3 = s3 / s2, the solutions of G / s2 = R + (t / d) n^T in the basis of the SVD are
                    x1 = sqrt(a (r1 + 1) / (w (r1 + r3))), x3 = sqrt(b (1 + r3) / (w (r1 + r3))),   [r^2 - 1 enters as (r - 1)(r + 1)]
                    sin = e sqrt(a (r1 + 1) b (1 + r3)) / (r1 + r3), cos = (1 + r1 r3) / (r1 + r3),  e = +1, -1
                    n = x1 v1 + e x3 v3, t = w (x1 u1 - e x3 u3), R = cos (u1 v1^T + u3 v3^T) + u2 v2^T + sin (u3 v1^T - u1 v3^T)
                and with each (R, t, n) its twin (R, -t, -n): four entries, also where the two pairs coincide (a = 0 or b = 0: t || n).
Rotation cut    w <= 2^-26: one solution, R = U V^T (the rotation nearest G / s2), t = n = 0, every vote 0.
n_distinct      the number of classes of entries; two entries are the same when |dR|, |dt| and |dn| (largest entry) are all under MERGE_TOL.
Votes           over the points i < n with finite coordinates, m = ((p - c) / f, 1) in float64:
                n_good[k]: i in the mask with n_k . m1 > 0 and (R_k n_k) . m2 > 0; n_off[k]: i outside the mask whose squared Sampson
                distance under E_k = [t_k / |t_k|]x R_k is <= (threshold / ((fx + fy) / 2))^2; n_mask: the finite points in the mask.
Rank            viable = n_good[k] >= ratio x max n_good; viable first, then n_off descending, then (with a hint) n_k . hint descending, then
                n_good descending, then trace R, n_z, n_y, n_x descending: properties of the solution, never the labelling of the SVD.
                `order_decided`: between neighbours in rank order the first key entry that differs does so by more than ORDER_MARGIN and no
                two entries are equal to the bit; only then is another implementation's order compared rank by rank (two coinciding pairs,
                or a normal with n_z = 0 when no point votes, are ordered by a rounding).
Ambiguity       1 iff no hint was given and the best candidate has a viable rival distinct from it (the first such in rank order) whose
                n_off is fewer than min_off below its own.  0 with a single solution.

The bound: |candidate - mpmath candidate| (largest entry of dR, d(t / |t|), dn) <= FACTOR x s, where s is that candidate's sensitivity: the
largest such change under relative perturbations of +-2^-53 of single entries of H, at 60 digits.  FACTOR is at most 10 x the worst ratio
measured, of this model on the CPU and of the kernel on the GPU (MEASURED).
"""
import math

import mpmath
import numpy as np

import essential_model as em

K = em.K
FULL_SEED = em.FULL_SEED
VO_E_NUMERIC = -6
ROT_CUT = 2.0 ** -26
# two entries closer than this in R, t and n are one solution.  The two pairs approach each other like sqrt(a): an a of a few roundings
# (2^-52) separates them by about 2^-26, so the tolerance lies well above that, and far under the O(1) separation of distinct solutions
MERGE_TOL = 2.0 ** -20
RATIO, THRESHOLD, MIN_OFF = 0.75, 1.0, 8
DIGITS = 60
DOT_MARGIN = 1e-9                 # no voting point of a GPU scene lies this close to zero in a visibility dot product
SAMPSON_MARGIN = 1e-6             # ... or this close (relative) to the Sampson threshold
ORDER_MARGIN = 1e-9               # the order of two neighbours is asserted where the key entry that decides it differs by more than this
# worst ratios error / s over every scene of SCENES_EXACT + the scaled and general-K variants: `model` by tests/test_hpose_model.py on the
# CPU, `kernel` by tests/test_gpu_hpose.py on an MI355X (both print theirs).  FACTOR is at most 10 x the larger.
# Measured: the model 6.624 (ground, general K), the kernel 5.520 (the same decomposition); 8 x 6.624 = 52.99, rounded up.
MEASURED = dict(model=6.624, kernel=5.520)
FACTOR = 53.0
K_GENERAL = np.array([[650.0, 0.0, 500.25], [0.0, 810.5, 140.75], [0.0, 0.0, 1.0]])      # unequal focal lengths, off-centre principal point


# =========================================================================================================================================
# scenes
# =========================================================================================================================================
def _project(X, R, t, Kc):
    p1 = X @ Kc.T
    Xc = X @ R.T + t
    p2 = Xc @ Kc.T
    return (p1[:, :2] / p1[:, 2:3]).astype(np.float32), (p2[:, :2] / p2[:, 2:3]).astype(np.float32)


def exact_scene(name, n=40, seed=FULL_SEED, Kc=K):
    """-> dict name, K, p1, p2 (n, 2) float32, R, t (metres), nrm (unit, n . X = d > 0 in view 1; None without a plane), d, X, H (exact, the
    float64 rounding of K (R + t n^T / d) K^-1 or K R K^-1).  `plane`, `fronto`, `pure_rotation`: essential_model.scene; `wall` a wall
    approached head-on (t || n); `ground` the plane Y = 1.65 under forward motion; `tiny` the plane scene with a baseline of 1e-6 m"""
    rng = np.random.default_rng([seed, 977])
    if name in ("plane", "fronto", "pure_rotation", "tiny"):
        s = em.scene("plane" if name == "tiny" else name, n, seed)
        R, t, X = s["R"], s["t"], s["X"]
        if name == "tiny":
            t = t / np.linalg.norm(t) * 1e-6
        nrm = dict(plane=np.array([-0.5, -0.3, 1.0]), tiny=np.array([-0.5, -0.3, 1.0]), fronto=np.array([0.0, 0.0, 1.0])).get(name)
        d = dict(plane=22.0, tiny=22.0, fronto=20.0).get(name)
    elif name == "wall":
        nrm, d = np.array([0.3, -0.1, 1.0]), 14.0
        R = em.syn.rodrigues(np.array([0.004, -0.01, 0.002]))
        X = np.stack([rng.uniform(-9, 9, n), rng.uniform(-3, 3, n), np.zeros(n)], 1)
        X[:, 2] = (d - X[:, :2] @ nrm[:2]) / nrm[2]
        t = -1.2 * (R @ nrm) / np.linalg.norm(nrm)          # towards the wall along the normal as view 2 sees it: t || R n, one pair
    elif name == "ground":
        nrm, d = np.array([0.0, 1.0, 0.0]), 1.65
        R = em.syn.rodrigues(np.array([0.002, 0.015, -0.001]))
        t = np.array([0.03, -0.01, -0.9])
        X = np.stack([rng.uniform(-6, 6, n), np.full(n, 1.65), rng.uniform(6, 30, n)], 1)
    else:
        raise KeyError(name)
    if nrm is not None:
        ln = float(np.linalg.norm(nrm))
        nrm, d = nrm / ln, d / ln
        G = R + np.outer(t, nrm) / d
    else:
        G, d = R, None
    p1, p2 = _project(X, R, t, Kc)
    return dict(name=name, K=Kc, p1=p1, p2=p2, R=R, t=t, nrm=nrm, d=d, X=X, H=Kc @ G @ np.linalg.inv(Kc))


SCENES_EXACT = ("plane", "fronto", "pure_rotation", "wall", "ground", "tiny")


def plane_off(seed=FULL_SEED):
    """`plane` (40) + the ten points of scene("general", 10, 5) under the plane scene's motion, exact H -> scene dict with `mask`"""
    s = exact_scene("plane", 40, seed)
    Xg = em.scene("general", 10, 5)["X"]
    q1, q2 = _project(Xg, s["R"], s["t"], s["K"])
    s.update(name="plane+off", p1=np.concatenate([s["p1"], q1]), p2=np.concatenate([s["p2"], q2]), X=np.concatenate([s["X"], Xg]),
             mask=np.concatenate([np.ones(40, np.uint8), np.zeros(10, np.uint8)]))
    return s


# =========================================================================================================================================
# float64 model
# =========================================================================================================================================
def g_matrix(Kc, H):
    """K^-1 H K of the H scaled by its largest entry, det > 0 -> (3, 3), or None (no solution)"""
    Kc, H = np.asarray(Kc, np.float64).reshape(3, 3), np.asarray(H, np.float64).reshape(3, 3)
    fx, fy, cx, cy = Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]
    big = np.abs(H).max()
    if not (np.isfinite(H).all() and np.isfinite([fx, fy, cx, cy]).all()) or big == 0.0 or fx == 0.0 or fy == 0.0:
        return None
    H = H / big
    M = np.stack([H[:, 0] * fx, H[:, 1] * fy, (H[:, 0] * cx + H[:, 1] * cy) + H[:, 2]], 1)
    G = np.stack([(M[0] - cx * M[2]) / fx, (M[1] - cy * M[2]) / fy, M[2]])
    det = (G[0, 0] * (G[1, 1] * G[2, 2] - G[1, 2] * G[2, 1]) - G[0, 1] * (G[1, 0] * G[2, 2] - G[1, 2] * G[2, 0])) + \
        G[0, 2] * (G[1, 0] * G[2, 1] - G[1, 1] * G[2, 0])
    if not (abs(det) > 0.0 and np.isfinite(det)):
        return None
    return -G if det < 0 else G


def jacobi_svd(G):
    """one-sided Jacobi on the columns (the sweeps of e5_decompose) -> s (3,) descending, U, V (columns; v3 = v1 x v2, u3 = u1 x u2)"""
    U, V = np.array(G, np.float64), np.eye(3)
    for _sweep in range(60):
        changed = False
        for p in range(2):
            for q in range(p + 1, 3):
                al, be, ga = U[:, p] @ U[:, p], U[:, q] @ U[:, q], U[:, p] @ U[:, q]
                if ga * ga > 4.930380657631324e-32 * (al * be):
                    changed = True
                    zeta = (be - al) / (2.0 * ga)
                    tt = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                    c = 1.0 / math.sqrt(1.0 + tt * tt)
                    s = c * tt
                    up, uq, vp, vq = U[:, p].copy(), U[:, q].copy(), V[:, p].copy(), V[:, q].copy()
                    U[:, p], U[:, q] = c * up - s * uq, s * up + c * uq
                    V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
        if not changed:
            break
    nn = np.array([U[:, j] @ U[:, j] for j in range(3)])
    order = sorted(range(3), key=lambda j: -nn[j])                      # stable: ties keep the column order
    sg = np.sqrt(nn[order])
    u1, u2 = U[:, order[0]] / sg[0], U[:, order[1]] / sg[1]
    v1, v2 = V[:, order[0]], V[:, order[1]]
    return sg, np.stack([u1, u2, np.cross(u1, u2)], 1), np.stack([v1, v2, np.cross(v1, v2)], 1)


def _solutions(sg, U, V, sqrt=math.sqrt, outer=np.outer, cut=ROT_CUT):
    """the formulas of the module docstring on any number type -> list of (R, t, n), sigma / s2"""
    s1, s2, s3 = sg
    a, b, w, r1, r3 = (s1 - s2) / s2, (s2 - s3) / s2, (s1 - s3) / s2, s1 / s2, s3 / s2
    u1, u2, u3 = U[:, 0], U[:, 1], U[:, 2]
    v1, v2, v3 = V[:, 0], V[:, 1], V[:, 2]
    if w <= cut:
        return [(outer(u1, v1) + outer(u2, v2) + outer(u3, v3), None, None)], (r1, r3)
    den = w * (r1 + r3)
    x1, x3 = sqrt(a * (r1 + 1) / den), sqrt(b * (1 + r3) / den)
    sn, cs = sqrt(a * (r1 + 1) * b * (1 + r3)) / (r1 + r3), (1 + r1 * r3) / (r1 + r3)
    out = []
    for e in (1, -1):
        n = x1 * v1 + (e * x3) * v3
        t = w * (x1 * u1 - (e * x3) * u3)
        R = cs * (outer(u1, v1) + outer(u3, v3)) + outer(u2, v2) + (e * sn) * (outer(u3, v1) - outer(u1, v3))
        out += [(R, t, n), (R, -t, -n)]
    return out, (r1, r3)


def decompose(Kc, H):
    """-> dict status, n_solutions (0, 1, 4), R (ns, 3, 3), t (ns, 3), n (ns, 3), sigma (3,) (s / s2), G (det > 0, scaled by s2); the entries
    in the order of the formulas (unranked)"""
    G = g_matrix(Kc, H)
    if G is None:
        return dict(status=VO_E_NUMERIC, n_solutions=0, R=np.zeros((0, 3, 3)), t=np.zeros((0, 3)), n=np.zeros((0, 3)), sigma=np.full(3, np.nan), G=None)
    sg, U, V = jacobi_svd(G)
    sol, (r1, r3) = _solutions(sg, U, V)
    z = np.zeros(3)
    R = np.stack([s[0] for s in sol])
    t = np.stack([z if s[1] is None else s[1] for s in sol])
    n = np.stack([z if s[2] is None else s[2] for s in sol])
    ok = np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(n).all()
    if not ok:
        return dict(status=VO_E_NUMERIC, n_solutions=0, R=np.zeros((0, 3, 3)), t=np.zeros((0, 3)), n=np.zeros((0, 3)), sigma=np.full(3, np.nan), G=None)
    return dict(status=0, n_solutions=len(sol), R=R, t=t, n=n, sigma=np.array([r1, 1.0, r3]), G=G / sg[1])


def same_entry(R, t, n, i, j, tol=MERGE_TOL):
    return bool(np.abs(R[i] - R[j]).max() < tol and np.abs(t[i] - t[j]).max() < tol and np.abs(n[i] - n[j]).max() < tol)


def n_distinct(R, t, n):
    reps = []
    for i in range(len(R)):
        if not any(same_entry(R, t, n, i, j) for j in reps):
            reps.append(i)
    return len(reps)


def normalise(p, Kc):
    p = np.asarray(p, np.float32).astype(np.float64).reshape(-1, 2)
    return (p[:, 0] - Kc[0, 2]) / Kc[0, 0], (p[:, 1] - Kc[1, 2]) / Kc[1, 1]


def essential_of(R, t):
    tu = t / math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    return np.stack([tu[1] * R[2] - tu[2] * R[1], tu[2] * R[0] - tu[0] * R[2], tu[0] * R[1] - tu[1] * R[0]])


def sampson(E, x1, y1, x2, y2):
    """the expression of e5_sampson"""
    a0, a1, a2 = E[0, 0] * x1 + E[0, 1] * y1 + E[0, 2], E[1, 0] * x1 + E[1, 1] * y1 + E[1, 2], E[2, 0] * x1 + E[2, 1] * y1 + E[2, 2]
    b0, b1 = E[0, 0] * x2 + E[1, 0] * y2 + E[2, 0], E[0, 1] * x2 + E[1, 1] * y2 + E[2, 1]
    num = x2 * a0 + y2 * a1 + a2
    with np.errstate(invalid="ignore", divide="ignore"):
        return num * num / (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1)


def votes(Kc, dec, p1, p2, mask=None, threshold=THRESHOLD):
    """-> dict n_good (ns,), n_off (ns,), n_mask, dots (the visibility dot products of the voting points, for the margin test), samp_rel
    (|d - thr2| / thr2 of the points outside the mask)"""
    ns = dec["n_solutions"]
    out = dict(n_good=np.zeros(ns, int), n_off=np.zeros(ns, int), n_mask=0, dots=np.zeros(0), samp_rel=np.zeros(0))
    if p1 is None or len(p1) == 0 or ns == 0:
        return out
    Kc = np.asarray(Kc, np.float64).reshape(3, 3)
    x1, y1 = normalise(p1, Kc)
    x2, y2 = normalise(p2, Kc)
    fin = np.isfinite(x1) & np.isfinite(y1) & np.isfinite(x2) & np.isfinite(y2)
    m = np.ones(len(x1), bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    tn = threshold / ((Kc[0, 0] + Kc[1, 1]) / 2.0)
    thr2 = tn * tn
    out["n_mask"] = int((fin & m).sum())
    if ns == 1:
        return out
    dots, rel = [], []
    for k in range(ns):
        R, t, n = dec["R"][k], dec["t"][k], dec["n"][k]
        rn = np.array([(R[i, 0] * n[0] + R[i, 1] * n[1]) + R[i, 2] * n[2] for i in range(3)])
        d1 = (n[0] * x1 + n[1] * y1) + n[2]
        d2 = (rn[0] * x2 + rn[1] * y2) + rn[2]
        with np.errstate(invalid="ignore"):
            out["n_good"][k] = int((fin & m & (d1 > 0) & (d2 > 0)).sum())
            sd = sampson(essential_of(R, t), x1, y1, x2, y2)
            out["n_off"][k] = int((fin & ~m & (sd <= thr2)).sum())
        dots += [d1[fin & m], d2[fin & m]]
        rel.append(np.abs(sd[fin & ~m] - thr2) / thr2)
    out["dots"], out["samp_rel"] = np.concatenate(dots), np.concatenate(rel)
    return out


def rank(dec, v, ratio=RATIO, min_off=MIN_OFF, hint=None):
    """-> dict order (indices into dec's entries, best first), viable (in rank order), ambiguous"""
    ns = dec["n_solutions"]
    if ns <= 1:
        return dict(order=list(range(ns)), viable=[True] * ns, ambiguous=0, order_decided=True)
    R, t, n = dec["R"], dec["t"], dec["n"]
    best = int(v["n_good"].max())
    viable = [bool(v["n_good"][k] >= ratio * best) for k in range(ns)]
    hd = [0.0 if hint is None else float((n[k, 0] * hint[0] + n[k, 1] * hint[1]) + n[k, 2] * hint[2]) for k in range(ns)]

    def key(k):
        return (1 if viable[k] else 0, int(v["n_off"][k]), hd[k], int(v["n_good"][k]), float((R[k, 0, 0] + R[k, 1, 1]) + R[k, 2, 2]),
                float(n[k, 2]), float(n[k, 1]), float(n[k, 0]))
    order = list(range(ns))
    for i in range(1, ns):                                  # insertion sort, an entry moves up only past a strictly smaller key
        j = i
        while j > 0 and key(order[j]) > key(order[j - 1]):
            order[j], order[j - 1] = order[j - 1], order[j]
            j -= 1
    # is the order above rounding?  Between neighbours the first key entry that differs at all must differ by more than ORDER_MARGIN (a
    # horizontal normal's n_z, or the traces of two coinciding pairs, differ by a rounding: their order is then nobody's to assert)
    decided = True
    for i in range(ns - 1):
        for x, y in zip(key(order[i]), key(order[i + 1])):
            if x != y:
                decided = decided and abs(x - y) > ORDER_MARGIN
                break
        else:
            decided = False                                 # two entries equal to the bit: pairs that coincide, and need not elsewhere
    amb = 0
    if hint is None and viable[order[0]]:
        for k in order[1:]:
            if viable[k] and not same_entry(R, t, n, order[0], k):
                amb = 1 if int(v["n_off"][order[0]]) - int(v["n_off"][k]) < min_off else 0
                break
    return dict(order=order, viable=[viable[k] for k in order], ambiguous=amb, order_decided=decided)


def hpose(Kc, H, p1=None, p2=None, mask=None, ratio=RATIO, threshold=THRESHOLD, min_off=MIN_OFF, hint=None):
    """the whole of vo_homography_decompose for one sequence -> dict status, n_solutions, n_distinct, ambiguous, n_mask, n_good, n_off (4,
    ranked, 0 beyond n_solutions), sigma, R (4, 3, 3), t (4, 3), n (4, 3) (ranked, NaN beyond n_solutions), rotation_only, order_decided, margins"""
    dec = decompose(Kc, H)
    ns = dec["n_solutions"]
    v = votes(Kc, dec, p1, p2, mask, threshold)
    rk = rank(dec, v, ratio, min_off, None if hint is None else np.asarray(hint, np.float64))
    R, t, n = np.full((4, 3, 3), np.nan), np.full((4, 3), np.nan), np.full((4, 3), np.nan)
    ng, no = np.zeros(4, int), np.zeros(4, int)
    for i, k in enumerate(rk["order"]):
        R[i], t[i], n[i], ng[i], no[i] = dec["R"][k], dec["t"][k], dec["n"][k], v["n_good"][k], v["n_off"][k]
    return dict(status=dec["status"], n_solutions=ns, n_distinct=n_distinct(dec["R"], dec["t"], dec["n"]), ambiguous=rk["ambiguous"],
                n_mask=v["n_mask"], n_good=ng, n_off=no, sigma=dec["sigma"], R=R, t=t, n=n, rotation_only=ns == 1, G=dec["G"], order_decided=rk["order_decided"],
                dots=v["dots"], samp_rel=v["samp_rel"])


def margins_ok(r):
    """the condition that keeps the GPU's counts exact: no visibility dot product within DOT_MARGIN of zero, no Sampson distance within
    SAMPSON_MARGIN (relative) of the threshold"""
    return bool((len(r["dots"]) == 0 or np.abs(r["dots"]).min() > DOT_MARGIN) and (len(r["samp_rel"]) == 0 or r["samp_rel"].min() > SAMPSON_MARGIN))


def variants():
    """(tag, K, H) of every decomposition the bound is measured on: the exact scenes, their H at another scale and sign, another K"""
    out = []
    for name in SCENES_EXACT:
        s = exact_scene(name, 40)
        out += [(name, s["K"], s["H"]), (name + " x -3.7", s["K"], -3.7 * s["H"]), (name + " x 1e6", s["K"], 1e6 * s["H"])]
        g = exact_scene(name, 40, Kc=K_GENERAL)
        out.append((name + " general K", g["K"], g["H"]))
    return out


def gpu_problems():
    """every (tag, K, H, p1, p2, mask, kw) whose counts tests/test_gpu_hpose.py compares for equality"""
    out = []
    for name in ("fronto", "plane", "pure_rotation", "wall", "ground"):
        s = exact_scene(name, 40)
        out.append((name, s["K"], s["H"], s["p1"], s["p2"], None, {}))
    s = exact_scene("plane", 40)
    r0 = hpose(s["K"], s["H"], s["p1"], s["p2"])
    for k in (0, 1):
        out.append(("plane hint %d" % k, s["K"], s["H"], s["p1"], s["p2"], None, dict(hint=r0["n"][k])))
    for f in (-3.7, 1e6):
        out.append(("plane x %g" % f, s["K"], f * s["H"], s["p1"], s["p2"], None, {}))
    o = plane_off()
    out.append(("plane+off", o["K"], o["H"], o["p1"], o["p2"], o["mask"], {}))
    m = np.ones(40, np.uint8)
    m[[3, 17, 30]] = 0
    out.append(("plane mask", s["K"], s["H"], s["p1"], s["p2"], m, {}))
    for n in (1, 63, 64, 65, 255, 256, 257):
        f = exact_scene("fronto", n)
        out.append(("fronto n=%d" % n, f["K"], f["H"], f["p1"], f["p2"], None, {}))
    g = exact_scene("plane", 40, Kc=K_GENERAL)
    out.append(("plane general K", g["K"], g["H"], g["p1"], g["p2"], None, {}))
    big = exact_scene("plane", 2000)
    out.append(("plane n=2000", big["K"], big["H"], big["p1"], big["p2"], None, {}))
    return out


# =========================================================================================================================================
# 60-digit restatement and the sensitivity
# =========================================================================================================================================
def _mp_decompose(Kc, Hm):
    """Hm an mpmath 3 x 3 -> list of (R (3, 3), t / |t| (3,) or None, n or None) as mpmath matrices, or None"""
    mp = mpmath.mp
    Km = mp.matrix(np.asarray(Kc, np.float64).reshape(3, 3).tolist())
    Km[0, 1] = 0
    G = mp.inverse(Km) * Hm * Km
    det = mp.det(G)
    if det == 0:
        return None
    if det < 0:
        G = -G
    U, S, Vt = mp.svd_r(G)
    V = Vt.T
    if mp.det(V) < 0:
        V[:, 2] = -V[:, 2]
        U[:, 2] = -U[:, 2]

    class _Cols:                                            # columns as numpy object vectors, so that _solutions serves both models
        def __init__(self, M):
            self.c = [np.array([M[i, j] for i in range(3)], object) for j in range(3)]

        def __getitem__(self, ix):
            return self.c[ix[1]]
    sol, _ = _solutions((S[0], S[1], S[2]), _Cols(U), _Cols(V), sqrt=mp.sqrt, outer=lambda x, y: np.array([[xi * yj for yj in y] for xi in x], object))
    out = []
    for R, t, n in sol:
        tu = None if t is None else t / mp.sqrt(sum(x * x for x in t))
        out.append((R, tu, n))
    return out


def _mp_dist(a, b):
    d = max(abs(x) for x in (a[0] - b[0]).ravel())
    if a[1] is not None and b[1] is not None:
        d = max(d, max(abs(x) for x in (a[1] - b[1])), max(abs(x) for x in (a[2] - b[2])))
    return d


def mp_model(Kc, H):
    """the decomposition of the float64 H at 60 digits -> list of dict R, tu (t / |t|), n (float64 roundings; tu = n = None for the
    rotation-only solution), s (the sensitivity, float)"""
    with mpmath.workdps(DIGITS):
        mp = mpmath.mp
        H = np.asarray(H, np.float64).reshape(3, 3)
        Hm = mp.matrix(H.tolist())
        base = _mp_decompose(Kc, Hm)
        if base is None:
            return []
        s = [mp.mpf(0)] * len(base)
        for i in range(3):
            for j in range(3):
                for sgn in (1, -1):
                    if H[i, j] == 0.0:
                        continue
                    Hp = Hm.copy()
                    Hp[i, j] = Hm[i, j] * (1 + sgn * mp.mpf(2) ** -53)
                    pert = _mp_decompose(Kc, Hp)
                    if pert is None:
                        continue
                    for k, c in enumerate(base):
                        s[k] = max(s[k], min(_mp_dist(c, q) for q in pert))
        f = lambda x: None if x is None else np.array(x, object).astype(np.float64)      # noqa: E731
        return [dict(R=f(c[0]), tu=f(c[1]), n=f(c[2]), s=float(s[k])) for k, c in enumerate(base)]


def candidate_error(R, t, n, c):
    """largest entry of dR, d(t / |t|), dn between one float64 candidate and one of mp_model's"""
    e = float(np.abs(R - c["R"]).max())
    if c["tu"] is not None:
        nt = np.linalg.norm(t)
        e = max(e, float(np.abs(t / nt - c["tu"]).max()) if nt > 0 else 1.0, float(np.abs(n - c["n"]).max()))
    return e


def worst_ratio(R, t, n, ns, ref):
    """every one of the ns candidates against its nearest of mp_model's `ref` -> the largest error / s; inf if the numbers differ"""
    if ns != len(ref):
        return math.inf
    worst = 0.0
    for k in range(ns):
        e, c = min(((candidate_error(R[k], t[k], n[k], c), c) for c in ref), key=lambda x: x[0])
        worst = max(worst, e / c["s"] if c["s"] > 0 else (0.0 if e == 0 else math.inf))
    return worst


def truth_error(r, s):
    """the smallest distance (largest entry of dR, d(t/d), dn) of a candidate of hpose's result r to the scene's (R, t / d, n)"""
    if s["nrm"] is None:
        return float(np.abs(r["R"][0] - s["R"]).max())
    td = s["t"] / s["d"]
    return min(max(float(np.abs(r["R"][k] - s["R"]).max()), float(np.abs(r["t"][k] - td).max()), float(np.abs(r["n"][k] - s["nrm"]).max()))
               for k in range(r["n_solutions"]))
