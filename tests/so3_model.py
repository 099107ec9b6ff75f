"""Bundle-adjustment linearisation and the SO(3) maps: an INDEPENDENT high-precision model.  TEST INFRASTRUCTURE, host only.

Everything the suite otherwise knows about the BA linearisation comes from oracle/ba_oracle.py, which shares the kernels' formulas (the same
closed-form Rodrigues, the same right Jacobian Jr, the same series switch at th2 < 1e-8, the same th < eps identity branch).  This file shares
none of them.  It imports neither ba_oracle nor vo_mi355x.so3 nor the cv2 stand-in, and it never writes a Jr:

  exp        R = I + (sin th / th) [r]x + ((1 - cos th) / th^2) [r]x^2, I at th = 0, in mpmath at DPS = 60 digits
  log        the exact logarithm (of the nearest rotation: the polar factor, by Newton's iteration in mpmath)
  project    dehom(K (R X + t)) for a general 3 x 3 K
  Jacobian   of the 2-vector error e = project - uv in (rvec, t, X): central differences with H = 1e-25 on the 60-digit projection (truncation
             ~ H^2 = 1e-50, rounding ~ 1e-60 / H = 1e-35 of the function's size)
  losses     scipy.optimize.least_squares' documentation: s = |e|^2, z = s / C^2, cost = 1/2 C^2 sum rho(z), weight = rho'(z)
                 linear   rho(z) = z                           huber    rho(z) = z if z <= 1 else 2 z^(1/2) - 1
                 soft_l1  rho(z) = 2 ((1 + z)^(1/2) - 1)       cauchy   rho(z) = ln(1 + z)            arctan   rho(z) = arctan(z)
  system     H = sum w J^T J, g = sum w J^T e in blocks Hpp, Hpl, Hll, gp, gl; the damped Schur system and one LM step as this project defines them
             (ba_oracle.schur_system / lm_step: damping lam * max(diag, 1e-12) on the diagonals of Hll and Hpp, S = Hpp_d - sum_j B_j M_j B_j^T,
             rhs = -gp + sum_j B_j M_j gl_j, dposes = S^-1 rhs, dpoints_j = -M_j (gl_j + B_j^T dposes)), solved in mpmath, rounded to float64 ONCE
  cost_ld    the cost in numpy.longdouble (no mpmath): what the GPU tests evaluate at the x a solve returns

The fixed cases (`case(name)`, deterministic; everything transcendental in their construction goes through mpmath):
  edge rotations  th in EDGE_ANGLES = {0, 1e-9, 9.9e-5 (th2 just below the series switch), 1.01e-4 (just above: 1 - cos cancels), 1e-3, 0.3,
                  pi - 1e-6, pi + 0.2, 2 pi - 1e-3 (Jr nearly singular), 7.5}, each about an axis of its own with every component >= 0.3
  scenes          cloud N(0, 4^2); t_i puts its centroid at about (x_i, 0.3, 30) in camera i; observations = projection + 0.3 px, ~8 % moved
                  10-40 px, ~15 % missing (NaN); points0 = cloud + 0.3; poses0 = poses + 0.02 in t, + 1e-3 in rvec where th >= 1e-3 (the
                  small angles stay exactly on their edge)
  A  W 10, N 25   one angle per slot; the general K; one landmark of points0 at camera-frame depth 0.5 in the th = 0.3 slot, one at depth -5 in
                  the th = pi + 0.2 slot; 25 = 2 x 12 + 1: one landmark in the last 12-landmark chunk
  B  W  9, N 13   A's angles without 7.5; synthetic.KITTI_K
  C  W  4, N 13   {0, 1.01e-4, pi - 1e-6, 0.3}; synthetic.KITTI_K
  D  W 12, N 25   A's angles + {9.9e-5 about another axis, 2.5}; the general K (windows above 10 slots: lane-per-observation kernels only)
tests/golden/gen_golden_so3.py writes them with the model's results to tests/golden/ba_so3_<case>.npz; `load(name)` reads one back without
mpmath.  S is symmetric to the last bit (the model forms its upper triangle and mirrors it), so the files hold that triangle.

What the float64 oracle achieves against this model (tests/test_so3_model.py measures it with oracle/ba_oracle.py and asserts
it with a factor 2; ORACLE_DEV below).  Block quantities: every Hpp[i], gp[i], Hll[j], gl[j] relative to its OWN largest magnitude, the worst
block; cost relative; S, rhs, dposes, dpoints norm-relative.  Worst over the six losses (five at C = 1, Huber at C = 2.5), floored at one
float64 ulp (the model's own rounding is half of one):
  case  cost     Hpp      gp       Hll      gl       S        rhs      dposes   dpoints  | e        Jp (per slot and column)  Jl
  A     2.4e-15  2.9e-13  2.5e-13  1.3e-13  9.6e-14  8.9e-14  1.0e-13  2.3e-13  5.2e-14  | 2.1e-15  3.9e-13                   6.9e-15
  B     2.6e-16  1.5e-13  1.7e-13  4.6e-14  3.4e-14  8.7e-14  9.6e-14  4.0e-13  3.7e-14  | 4.5e-15  2.4e-13                   1.7e-15
  C     3.2e-16  8.3e-14  2.5e-13  6.8e-14  4.9e-14  1.2e-13  1.6e-13  6.7e-13  1.1e-13  | 7.2e-15  2.4e-13                   4.7e-16
  D     1.8e-15  3.0e-13  2.4e-13  1.3e-13  9.6e-14  7.2e-14  1.6e-13  1.0e-12  2.0e-13  | 2.9e-15  3.5e-13                   8.6e-15
(oracle/ba_oracle.py alone: loss_normal_equations, schur_system, lm_step, and loss_cost as a second evaluation of the cost; its exp is within
3.4e-16 of the model's entry by entry.  `mutant_probe` without a mutation has a table of its own, HELPER_DEV, which sets no tolerance.)
Every GPU tolerance of tests/test_gpu_ba_so3.py is 8 x the value here, capped at the suite's existing bounds (CAPS).  The smallest structural
error is orders above: MUTANT_MARGIN lists by how much the three mutated linearisations of `mutant_probe` miss the same comparison.
so3.rodrigues_mat_to_vec against the exact log outside OpenCV's snap zones, as a rotation angle: SO3_LOG_DEV (it grows like ulp / sin th, the
conditioning of acos and of the antisymmetric part).
"""
import os

import numpy as np

try:                                      # the GPU tests read the fixtures and cost_ld only: no mpmath there
    import mpmath as mp
except ImportError:                       # pragma: no cover
    mp = None

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DPS = 60
H_STEP = "1e-25"
LAM = 1e-3
LOSSES = ("huber", "linear", "soft_l1", "cauchy", "arctan")
LOSS_RUNS = tuple((l, l, 1.0) for l in LOSSES) + (("huber_c2.5", "huber", 2.5),)          # (tag in the fixture, loss, C)
PER_LOSS = ("cost", "Hpp", "gp", "Hll", "gl", "S", "rhs", "dposes", "dpoints")
BLOCK_KEYS = ("Hpp", "gp", "Hll", "gl")
NORM_KEYS = ("S", "rhs", "dposes", "dpoints")
CAPS = {"Hpp": 1e-10, "gp": 1e-10, "Hll": 1e-10, "gl": 1e-10, "cost": 1e-12, "S": 1e-8, "rhs": 1e-8, "dposes": 1e-6, "dpoints": 1e-6}
EPS = float(np.finfo(np.float64).eps)

EDGE_ANGLES = (0.0, 1e-9, 9.9e-5, 1.01e-4, 1e-3, 0.3, np.pi - 1e-6, np.pi + 0.2, 2 * np.pi - 1e-3, 7.5)
LOG_ANGLES = (1e-6, 1e-4, np.pi - 1e-4, np.pi - 1e-6)              # the log's own edges: either side of OpenCV's snap zones (sin th < 1e-5)
PIPE_ANGLES = (1e-6, 1e-4, 0.3, 2.5, np.pi - 1e-4, np.pi - 1e-6, np.pi + 0.2)   # the closed loop's trajectory (tests/test_gpu_pipe_fuzz.py), axis k for angle k
KITTI_K = np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]])       # = synthetic.KITTI_K (tests/test_so3_model.py)
GENERAL_K = np.array([[718.856, 0.7, 607.19], [0.0, 715.2, 185.2], [1e-4, -2e-4, 1.0]])

# measured by tests/test_so3_model.py::test_oracle_against_the_fixtures (see the docstring)
ORACLE_DEV = {
    "A": {"e": 2.1e-15, "Jp": 3.9e-13, "Jl": 6.9e-15, "cost": 2.4e-15, "Hpp": 2.9e-13, "gp": 2.5e-13, "Hll": 1.3e-13, "gl": 9.6e-14, "S": 8.9e-14, "rhs": 1.0e-13, "dposes": 2.3e-13, "dpoints": 5.2e-14},
    "B": {"e": 4.5e-15, "Jp": 2.4e-13, "Jl": 1.7e-15, "cost": 2.6e-16, "Hpp": 1.5e-13, "gp": 1.7e-13, "Hll": 4.6e-14, "gl": 3.4e-14, "S": 8.7e-14, "rhs": 9.6e-14, "dposes": 4.0e-13, "dpoints": 3.7e-14},
    "C": {"e": 7.2e-15, "Jp": 2.4e-13, "Jl": 4.7e-16, "cost": 3.2e-16, "Hpp": 8.3e-14, "gp": 2.5e-13, "Hll": 6.8e-14, "gl": 4.9e-14, "S": 1.2e-13, "rhs": 1.6e-13, "dposes": 6.7e-13, "dpoints": 1.1e-13},
    "D": {"e": 2.9e-15, "Jp": 3.5e-13, "Jl": 8.6e-15, "cost": 1.8e-15, "Hpp": 3.0e-13, "gp": 2.4e-13, "Hll": 1.3e-13, "gl": 9.6e-14, "S": 7.2e-14, "rhs": 1.6e-13, "dposes": 1.0e-12, "dpoints": 2.0e-13},
}
# the same for `mutant_probe` without a mutation (test_helper_without_a_mutation_against_the_fixtures): the float64 linearisation the mutants are
# made from.  It restates the device's formulas, so it sets NO tolerance; its own record only shows that the helper is right
HELPER_DEV = {
    "A": {"cost": 2.6e-15, "Hpp": 2.9e-13, "gp": 2.5e-13, "Hll": 4.8e-14, "gl": 3.9e-14, "S": 8.8e-14, "rhs": 9.0e-14, "dposes": 3.4e-13, "dpoints": 4.9e-13},
    "B": {"cost": 4.1e-16, "Hpp": 1.5e-13, "gp": 1.7e-13, "Hll": 4.6e-14, "gl": 3.4e-14, "S": 8.6e-14, "rhs": 6.5e-14, "dposes": 4.7e-13, "dpoints": 4.0e-14},
    "C": {"cost": 4.6e-16, "Hpp": 8.2e-14, "gp": 2.4e-13, "Hll": 7.0e-14, "gl": 5.0e-14, "S": 1.2e-13, "rhs": 1.6e-13, "dposes": 1.6e-12, "dpoints": 1.1e-13},
    "D": {"cost": 1.0e-15, "Hpp": 3.0e-13, "gp": 2.1e-13, "Hll": 1.1e-13, "gl": 8.8e-14, "S": 7.7e-14, "rhs": 1.8e-13, "dposes": 9.0e-13, "dpoints": 5.2e-13},
}
# |so3.rodrigues_mat_to_vec - exact log| as a rotation angle at the angles of EDGE_ANGLES + LOG_ANGLES + PIPE_ANGLES with |sin th| >= 1e-5, measured likewise
SO3_LOG_DEV = {9.9e-5: 9.9e-14, 1.01e-4: 1.9e-12, 1e-3: 7.8e-15, 0.3: 6.3e-16, np.pi + 0.2: 8.9e-16, 2 * np.pi - 1e-3: 2.3e-13, 7.5: 5.5e-16,
               1e-4: 2.6e-13, np.pi - 1e-4: 2.5e-12, 2.5: 3.0e-16}
# largest entry of |so3.rodrigues_vec_to_mat - exp| and |ba_oracle.rodrigues_exp - exp| over EDGE_ANGLES + LOG_ANGLES
SO3_EXP_DEV = 3.4e-16
# smallest factor by which a mutated linearisation exceeds a GPU tolerance it must miss (tests/test_so3_model.py::test_mutants_fail_the_probe_comparison)
MUTANT_MARGIN = {"a_z": 4.8e11, "b_xy": 4.7e11, "R_transposed": 1.5e12}


def gpu_tol(name, key):
    """8 x the recorded CPU value, capped at the suite's bound for the quantity"""
    return min(8.0 * ORACLE_DEV[name][key], CAPS[key])


# ================================================================================================
# mpmath: exp, log, projection, Jacobian by central differences
# ================================================================================================
def _mpf(v):
    return [mp.mpf(float(x)) for x in np.asarray(v, np.float64).reshape(-1)]


def _exp(r):
    """r: 3 mpf -> 3 x 3 list.  [r]x^2 = r r^T - th^2 I written out"""
    x, y, z = r
    th2 = x * x + y * y + z * z
    one = mp.mpf(1)
    if th2 == 0:
        return [[one, 0, 0], [0, one, 0], [0, 0, one]]
    th = mp.sqrt(th2)
    a, b = mp.sin(th) / th, (one - mp.cos(th)) / th2
    return [[one - b * (y * y + z * z), -a * z + b * x * y, a * y + b * x * z],
            [a * z + b * x * y, one - b * (x * x + z * z), -a * x + b * y * z],
            [-a * y + b * x * z, a * x + b * y * z, one - b * (x * x + y * y)]]


def exp(r, dps=DPS):
    """rvec -> R, float64 rounding of the 60-digit matrix"""
    with mp.workdps(dps):
        return np.array([[float(v) for v in row] for row in _exp(_mpf(r))])


def _polar(R):
    """nearest rotation of a matrix close to one: X <- (X + X^-T) / 2"""
    X = mp.matrix(R)
    for _ in range(60):
        Y = (X + (X ** -1).T) / 2
        d = max(abs(Y[i, j] - X[i, j]) for i in range(3) for j in range(3))
        X = Y
        if d < mp.mpf(10) ** (-mp.mp.dps + 5):
            break
    return X


def _log(R):
    """the exact logarithm of a rotation (mp.matrix), principal branch |r| <= pi.  Near pi the antisymmetric part fades: the axis comes from the
    symmetric part, its sign from what is left of the antisymmetric one (at th = pi exactly both signs are logarithms)"""
    v = [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]
    s = mp.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) / 2
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
    th = mp.atan2(s, c)
    if s > mp.mpf(10) ** (-mp.mp.dps // 3):
        return [x * th / (2 * s) for x in v]
    if c > 0:
        return [x / 2 for x in v]                                  # th / sin th = 1 to working precision
    # th ~ pi: (R + R^T) / 2 = cos th I + (1 - cos th) k k^T
    M = [[((R[i, j] + R[j, i]) / 2 - (c if i == j else 0)) / (1 - c) for j in range(3)] for i in range(3)]
    i = max(range(3), key=lambda q: M[q][q])
    k = [M[i][j] / mp.sqrt(M[i][i]) for j in range(3)]
    sgn = 1
    if s > 0:
        sgn = 1 if (k[0] * v[0] + k[1] * v[1] + k[2] * v[2]) >= 0 else -1
    return [sgn * x * th for x in k]


def log(R, dps=DPS):
    """R (float64, a rotation to rounding error) -> rvec of the nearest rotation, float64 rounding of the 60-digit vector"""
    with mp.workdps(dps):
        Rm = _polar([[mp.mpf(float(x)) for x in row] for row in np.asarray(R, np.float64).reshape(3, 3)])
        return np.array([float(x) for x in _log(Rm)])


def rotation_distance(ra, rb, dps=DPS):
    """angle of exp(ra)^T exp(rb)"""
    with mp.workdps(dps):
        A, B = mp.matrix(_exp(_mpf(ra))), mp.matrix(_exp(_mpf(rb)))
        r = _log(A.T * B)
        return float(mp.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]))


def _project(K, q):
    """K: 9 mpf, q = (rvec, t, X): 9 mpf -> (u, v)"""
    R = _exp(q[0:3])
    X = q[6:9]
    c = [R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + q[3 + i] for i in range(3)]
    p = [K[3 * i] * c[0] + K[3 * i + 1] * c[1] + K[3 * i + 2] * c[2] for i in range(3)]
    return p[0] / p[2], p[1] / p[2]


def project(K, pose, X, dps=DPS):
    with mp.workdps(dps):
        u, v = _project(_mpf(K), _mpf(pose) + _mpf(X))
        return np.array([float(u), float(v)])


def _error_and_jacobian(K, q, uv, h):
    """e (2 mpf), J 2 x 9 (d e / d (rvec, t, X)) by central differences"""
    u, v = _project(K, q)
    J = [[None] * 9, [None] * 9]
    for k in range(9):
        qp, qm = list(q), list(q)
        qp[k] = q[k] + h; qm[k] = q[k] - h
        (up, vp), (um, vm) = _project(K, qp), _project(K, qm)
        J[0][k], J[1][k] = (up - um) / (2 * h), (vp - vm) / (2 * h)
    return [u - uv[0], v - uv[1]], J


def _rho(z, loss):
    """(rho(z), rho'(z)) as scipy.optimize.least_squares documents its losses"""
    one = mp.mpf(1)
    if loss == "linear":
        return z, one
    if loss == "huber":
        return (z, one) if z <= 1 else (2 * mp.sqrt(z) - 1, 1 / mp.sqrt(z))
    if loss == "soft_l1":
        return 2 * (mp.sqrt(1 + z) - 1), 1 / mp.sqrt(1 + z)
    if loss == "cauchy":
        return mp.log(1 + z), 1 / (1 + z)
    if loss == "arctan":
        return mp.atan(z), 1 / (1 + z * z)
    raise ValueError(loss)


# ================================================================================================
# the linearisation of a problem, its normal equations, the damped Schur system and one LM step
# ================================================================================================
def linearise(K, poses, points, obs, dps=DPS, h=H_STEP):
    """-> dict (i, j) -> (e, J) in mpmath numbers of precision dps for every observation present"""
    out = {}
    with mp.workdps(dps):
        hm = mp.mpf(h)
        Km, P, X = _mpf(K), [_mpf(p) for p in poses], [_mpf(x) for x in points]
        W, N = obs.shape[:2]
        for i in range(W):
            for j in range(N):
                if obs[i, j, 0] == obs[i, j, 0]:
                    out[i, j] = _error_and_jacobian(Km, P[i] + X[j], _mpf(obs[i, j]), hm)
    return out


def jacobians_f64(lin, W, N):
    e, Jp, Jl = np.zeros((W, N, 2)), np.zeros((W, N, 2, 6)), np.zeros((W, N, 2, 3))
    for (i, j), (ee, J) in lin.items():
        for k in range(2):
            e[i, j, k] = float(ee[k])
            Jp[i, j, k] = [float(x) for x in J[k][:6]]
            Jl[i, j, k] = [float(x) for x in J[k][6:]]
    return e, Jp, Jl


def _inv3(A):
    (a, b, c), (d, e, f), (g, h, i) = A
    co = [[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f], [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = a * co[0][0] + b * co[1][0] + c * co[2][0]
    return [[x / det for x in row] for row in co]


def _solve(S, b):
    return list(mp.lu_solve(mp.matrix(S), mp.matrix(b)))


def system(lin, W, N, loss, C, lam=LAM, dps=DPS):
    """-> dict of float64 arrays: cost, Hpp [W,6,6], gp [W,6], Hll [N,3,3], gl [N,3], Hpl [W,N,6,3], S [6W,6W], rhs [6W], dposes [W,6], dpoints [N,3]"""
    with mp.workdps(dps):
        zero = mp.mpf(0)
        Cm = mp.mpf(float(C)); C2 = Cm * Cm
        lamm = mp.mpf(float(lam)); floor = mp.mpf("1e-12")
        Hpp = [[[zero] * 6 for _ in range(6)] for _ in range(W)]
        gp = [[zero] * 6 for _ in range(W)]
        Hll = [[[zero] * 3 for _ in range(3)] for _ in range(N)]
        gl = [[zero] * 3 for _ in range(N)]
        Hpl = {}
        cost = zero
        for (i, j), (e, J) in sorted(lin.items()):
            s = e[0] * e[0] + e[1] * e[1]
            rho, w = _rho(s / C2, loss)
            cost += C2 * rho / 2
            for a in range(9):
                ga = w * (J[0][a] * e[0] + J[1][a] * e[1])
                if a < 6:
                    gp[i][a] += ga
                else:
                    gl[j][a - 6] += ga
            B = [[zero] * 3 for _ in range(6)]
            for a in range(9):
                for b in range(9):
                    hab = w * (J[0][a] * J[0][b] + J[1][a] * J[1][b])
                    if a < 6 and b < 6:
                        Hpp[i][a][b] += hab
                    elif a >= 6 and b >= 6:
                        Hll[j][a - 6][b - 6] += hab
                    elif a < 6:
                        B[a][b - 6] = hab
            Hpl[i, j] = B
        # damped landmark blocks and their inverses
        M = []
        for j in range(N):
            A = [row[:] for row in Hll[j]]
            for k in range(3):
                A[k][k] += lamm * max(Hll[j][k][k], floor)
            M.append(_inv3(A))
        z = [[sum(M[j][a][b] * gl[j][b] for b in range(3)) for a in range(3)] for j in range(N)]
        n = 6 * W
        S = [[zero] * n for _ in range(n)]
        rhs = [zero] * n
        for i in range(W):
            for a in range(6):
                for b in range(6):
                    S[6 * i + a][6 * i + b] = Hpp[i][a][b]
                S[6 * i + a][6 * i + a] += lamm * max(Hpp[i][a][a], floor)
                rhs[6 * i + a] = -gp[i][a]
        BM = {ij: [[sum(B[a][c] * M[ij[1]][c][d] for c in range(3)) for d in range(3)] for a in range(6)] for ij, B in Hpl.items()}
        for (i, j), bm in BM.items():
            for a in range(6):
                rhs[6 * i + a] += sum(Hpl[i, j][a][c] * z[j][c] for c in range(3))
            for k in range(i, W):
                if (k, j) not in Hpl:
                    continue
                Bk = Hpl[k, j]
                for a in range(6):
                    for b in range(6):
                        if k == i and b < a:
                            continue
                        S[6 * i + a][6 * k + b] -= bm[a][0] * Bk[b][0] + bm[a][1] * Bk[b][1] + bm[a][2] * Bk[b][2]
        for p in range(n):
            for q in range(p):
                S[p][q] = S[q][p]
        dp = _solve(S, rhs)
        dl = []
        for j in range(N):
            t = [gl[j][c] + sum(Hpl[i, j][a][c] * dp[6 * i + a] for i in range(W) if (i, j) in Hpl for a in range(6)) for c in range(3)]
            dl.append([-sum(M[j][a][c] * t[c] for c in range(3)) for a in range(3)])
        f = lambda a: np.vectorize(float, otypes=[np.float64])(np.array(a, dtype=object))      # the ONE rounding to float64
        Hpl_f = np.zeros((W, N, 6, 3))
        for (i, j), B in Hpl.items():
            Hpl_f[i, j] = f(B)
        return dict(cost=float(cost), Hpp=f(Hpp), gp=f(gp), Hll=f(Hll), gl=f(gl), Hpl=Hpl_f, S=f(S), rhs=f(rhs),
                    dposes=f(dp).reshape(W, 6), dpoints=f(dl))


# ================================================================================================
# cost in numpy.longdouble (run time: no mpmath)
# ================================================================================================
def cost_ld(K, poses, points, obs, loss="huber", C=1.0):
    """1/2 C^2 sum rho(|e|^2 / C^2) over the observations present, evaluated in numpy.longdouble -> float"""
    L = np.longdouble
    K, poses, points, obs = (np.asarray(a, L) for a in (K, poses, points, obs))
    W = obs.shape[0]
    C2 = L(C) * L(C)
    total = L(0)
    for i in range(W):
        x, y, z = poses[i, :3]
        th2 = x * x + y * y + z * z
        if th2 == 0:
            a, b = L(1), L(0.5)
        else:
            th = np.sqrt(th2)
            a = np.sin(th) / th
            hs = np.sin(th / 2)
            b = 2 * hs * hs / th2                                        # (1 - cos th) / th^2 without the cancellation
        R = np.array([[1 - b * (y * y + z * z), -a * z + b * x * y, a * y + b * x * z],
                      [a * z + b * x * y, 1 - b * (x * x + z * z), -a * x + b * y * z],
                      [-a * y + b * x * z, a * x + b * y * z, 1 - b * (x * x + y * y)]], L)
        m = ~np.isnan(obs[i, :, 0])
        p = (points[m] @ R.T + poses[i, 3:]) @ K.T
        e = p[:, :2] / p[:, 2:3] - obs[i][m]
        zz = (e * e).sum(-1) / C2
        if loss == "linear":
            rho = zz
        elif loss == "huber":
            rho = np.where(zz <= 1, zz, 2 * np.sqrt(zz) - 1)
        elif loss == "soft_l1":
            rho = 2 * zz / (np.sqrt(1 + zz) + 1)                         # = 2 (sqrt(1 + z) - 1)
        elif loss == "cauchy":
            rho = np.log1p(zz)
        elif loss == "arctan":
            rho = np.arctan(zz)
        else:
            raise ValueError(loss)
        total += rho.sum(dtype=L)
    return float(C2 * total / 2)


# ================================================================================================
# the fixed cases
# ================================================================================================
def _axes(n):
    """unit axes, every component >= 0.3 in magnitude (components drawn from +-[0.45, 0.75]: >= 0.45 / (sqrt(3) 0.75) = 0.346 after scaling)"""
    rng = np.random.default_rng(4242)
    a = rng.uniform(0.45, 0.75, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    return a / np.sqrt((a * a).sum(-1))[:, None]


AXES = _axes(12)
_SPECS = {
    #        angles (with the index of each one's axis)                                    N   K       seed  special landmarks
    "A": (list(zip(EDGE_ANGLES, range(10))), 25, "general", 11, True),
    "B": (list(zip(EDGE_ANGLES[:9], range(9))), 13, "kitti", 12, False),
    "C": ([(0.0, 0), (1.01e-4, 3), (np.pi - 1e-6, 6), (0.3, 5)], 13, "kitti", 13, False),
    "D": (list(zip(EDGE_ANGLES, range(10))) + [(9.9e-5, 10), (2.5, 11)], 25, "general", 14, True),
}
CASES = tuple(sorted(_SPECS))
NEAR_PLANE = (5, 3, 0.5)         # (slot: th = 0.3, landmark, camera-frame depth) in A and D
BEHIND = (7, 17, -5.0)           # (slot: th = pi + 0.2, landmark, depth)


def case(name):
    """-> dict(K, poses0 [W,6], points0 [N,3], obs [W,N,2], angles [W]): the inputs of case `name`.  Needs mpmath (exact projections)."""
    spec, N, kname, seed, special = _SPECS[name]
    W = len(spec)
    rng = np.random.default_rng(seed)
    K = GENERAL_K.copy() if kname == "general" else KITTI_K.copy()
    angles = np.array([a for a, _ in spec])
    X = rng.normal(0.0, 4.0, (N, 3))
    poses = np.zeros((W, 6))
    for i, (th, ax) in enumerate(spec):
        poses[i, :3] = th * AXES[ax]
        R = exp(poses[i, :3])
        poses[i, 3:] = np.array([0.5 * (i - (W - 1) / 2), 0.3, 30.0]) - R @ X.mean(0)
    obs = np.zeros((W, N, 2))
    for i in range(W):
        for j in range(N):
            obs[i, j] = project(K, poses[i], X[j])
    obs += rng.normal(0.0, 0.3, obs.shape)
    out = rng.random((W, N)) < 0.08
    d = rng.normal(0.0, 1.0, (W, N, 2))
    d = d / np.sqrt((d * d).sum(-1))[..., None] * rng.uniform(10.0, 40.0, (W, N, 1))
    obs[out] += d[out]
    miss = rng.random((W, N)) < 0.15
    if special:
        miss[NEAR_PLANE[0], NEAR_PLANE[1]] = miss[BEHIND[0], BEHIND[1]] = False
    for j in range(N):                       # every landmark keeps three observations, every slot three landmarks
        for i in range(W):
            if (~miss[:, j]).sum() >= 3:
                break
            miss[i, j] = False
    for i in range(W):
        for j in range(N):
            if (~miss[i]).sum() >= 3:
                break
            miss[i, j] = False
    obs[miss] = np.nan
    points0 = X + rng.normal(0.0, 0.3, (N, 3))
    poses0 = poses.copy()
    poses0[:, 3:] += rng.normal(0.0, 0.02, (W, 3))
    dr = rng.normal(0.0, 1e-3, (W, 3))
    poses0[angles >= 1e-3, :3] += dr[angles >= 1e-3]
    if special:
        for (i, j, depth), xy in ((NEAR_PLANE, (0.1, -0.05)), (BEHIND, (1.5, -0.8))):
            R = exp(poses0[i, :3])
            points0[j] = R.T @ (np.array([xy[0], xy[1], depth]) - poses0[i, 3:])
    return dict(K=K, poses0=poses0, points0=points0, obs=obs, angles=angles)


def build_fixture(name, dps=DPS, h=H_STEP):
    """the arrays of tests/golden/ba_so3_<name>.npz"""
    c = case(name)
    W, N = c["obs"].shape[:2]
    lin = linearise(c["K"], c["poses0"], c["points0"], c["obs"], dps, h)
    e, Jp, Jl = jacobians_f64(lin, W, N)
    out = dict(c, e=e, Jp=Jp, Jl=Jl, lam=np.float64(LAM))
    iu = np.triu_indices(6 * W)
    for tag, loss, C in LOSS_RUNS:
        s = system(lin, W, N, loss, C, LAM, dps)
        for k in PER_LOSS:
            out[tag + "__" + k] = np.float64(s[k]) if k != "S" else s["S"][iu]
    return out


def path(name):
    return os.path.join(GOLDEN, "ba_so3_%s.npz" % name)


def load(name):
    """-> dict(K, poses0, points0, obs, angles, e, Jp, Jl, lam, runs = {tag: dict(loss, C, cost, Hpp, ..., S (full), ...)})"""
    with np.load(path(name)) as z:
        raw = {k: z[k] for k in z.files}
    out = {k: v for k, v in raw.items() if "__" not in k}
    W = out["obs"].shape[0]
    iu = np.triu_indices(6 * W)
    out["runs"] = {}
    for tag, loss, C in LOSS_RUNS:
        r = dict(loss=loss, C=C)
        for k in PER_LOSS:
            v = raw[tag + "__" + k]
            if k == "S":
                S = np.zeros((6 * W, 6 * W))
                S[iu] = v
                v = S + np.triu(S, 1).T
            r[k] = float(v) if k == "cost" else v
        out["runs"][tag] = r
    return out


# ================================================================================================
# the comparison every probe goes through (the oracle on the CPU, the device, the mutants)
# ================================================================================================
def deviations(got, want):
    """-> {quantity: deviation}: block quantities by their worst block (each block relative to its OWN largest magnitude, so that the landmark
    next to a camera plane cannot mask the rest), the cost relative, the reduced system and the step norm-relative"""
    d = {"cost": abs(got["cost"] - want["cost"]) / abs(want["cost"])}
    for k in BLOCK_KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        ax = tuple(range(1, w.ndim))
        d[k] = float((np.abs(g - w).max(axis=ax) / np.abs(w).max(axis=ax)).max())
    for k in NORM_KEYS:
        g, w = np.asarray(got[k]).reshape(-1), np.asarray(want[k]).reshape(-1)
        d[k] = float(np.linalg.norm(g - w) / np.linalg.norm(w))
    return d


def check_probe(got, want, tol, what=""):
    """assert deviations(got, want)[k] <= tol[k] for every quantity; -> the deviations"""
    d = deviations(got, want)
    print(what, " ".join("%s %.1e/%.1e" % (k, d[k], tol[k]) for k in d))
    bad = {k: (d[k], tol[k]) for k in d if not d[k] <= tol[k]}
    assert not bad, (what, bad)
    return d


# ================================================================================================
# mutants: a float64 analytic linearisation with ONE term wrong (what the comparison must reject)
# ================================================================================================
MUTANTS = ("a_z", "b_xy", "R_transposed")


def mutant_probe(fx, loss, C, mutant=None, lam=LAM):
    """The quantities of a probe from an analytic float64 linearisation written like the device's (R, the right Jacobian Jr with a, b, the
    chain through [X]x), with one term negated: 'a_z' the a z term of Jr[0][1], 'b_xy' the b x y term of Jr[0][1], 'R_transposed' R^T for R.
    mutant=None is the correct linearisation (it must PASS the comparison: the helper itself is right)."""
    K, poses, points, obs = fx["K"], fx["poses0"], fx["points0"], fx["obs"]
    W, N = obs.shape[:2]
    Hpp, gp, Hll, gl = np.zeros((W, 6, 6)), np.zeros((W, 6)), np.zeros((N, 3, 3)), np.zeros((N, 3))
    Hpl = np.zeros((W, N, 6, 3))
    cost = 0.0
    for i in range(W):
        x, y, z = poses[i, :3]
        th2 = x * x + y * y + z * z
        th = np.sqrt(th2)
        if th2 < 1e-8:
            a, b, sa = 0.5 - th2 / 24, 1.0 / 6 - th2 / 120, 1.0 - th2 / 6
        else:
            a, b, sa = (1 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th), np.sin(th) / th
        Sx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0.0]])
        R = np.eye(3) + sa * Sx + a * (Sx @ Sx)
        Jr = np.eye(3) - a * Sx + b * (Sx @ Sx)
        if mutant == "a_z":
            Jr[0, 1] -= 2 * a * z
        elif mutant == "b_xy":
            Jr[0, 1] -= 2 * b * x * y
        elif mutant == "R_transposed":
            R = R.T.copy()
        elif mutant is not None:
            raise ValueError(mutant)
        for j in range(N):
            if obs[i, j, 0] != obs[i, j, 0]:
                continue
            X = points[j]
            p = K @ (R @ X + poses[i, 3:])
            uv = p[:2] / p[2]
            e = uv - obs[i, j]
            A = (K[:2] - uv[:, None] * K[2][None, :]) / p[2]
            Xx = np.array([[0, -X[2], X[1]], [X[2], 0, -X[0]], [-X[1], X[0], 0.0]])
            J = np.concatenate([-A @ R @ Xx @ Jr, A, A @ R], axis=1)            # 2 x 9
            s = e @ e
            zz = s / (C * C)
            if loss == "linear":
                rho, w = zz, 1.0
            elif loss == "huber":
                rho, w = (zz, 1.0) if zz <= 1 else (2 * np.sqrt(zz) - 1, 1 / np.sqrt(zz))
            elif loss == "soft_l1":
                rho, w = 2 * (np.sqrt(1 + zz) - 1), 1 / np.sqrt(1 + zz)
            elif loss == "cauchy":
                rho, w = np.log1p(zz), 1 / (1 + zz)
            else:
                rho, w = np.arctan(zz), 1 / (1 + zz * zz)
            cost += 0.5 * C * C * rho
            H, g = w * J.T @ J, w * J.T @ e
            Hpp[i] += H[:6, :6]; gp[i] += g[:6]; Hll[j] += H[6:, 6:]; gl[j] += g[6:]; Hpl[i, j] = H[:6, 6:]
    i3, i6 = np.arange(3), np.arange(6)
    Hd = Hll.copy()
    Hd[:, i3, i3] += lam * np.maximum(Hll[:, i3, i3], 1e-12)
    M = np.linalg.inv(Hd)
    S = np.zeros((6 * W, 6 * W))
    for i in range(W):
        blk = Hpp[i].copy()
        blk[i6, i6] += lam * np.maximum(Hpp[i][i6, i6], 1e-12)
        S[6 * i:6 * i + 6, 6 * i:6 * i + 6] = blk
    B = Hpl.transpose(0, 2, 1, 3).reshape(6 * W, N, 3)
    S -= np.einsum('pnc,ncd,qnd->pq', B, M, B)
    zl = np.einsum('ncd,nd->nc', M, gl)
    rhs = -gp.reshape(-1) + np.einsum('pnc,nc->p', B, zl)
    dp = np.linalg.solve(S, rhs)
    dl = -zl - np.einsum('ncd,nd->nc', M, np.einsum('pnc,p->nc', B, dp))
    return dict(cost=cost, Hpp=Hpp, gp=gp, Hll=Hll, gl=gl, S=S, rhs=rhs, dposes=dp.reshape(W, 6), dpoints=dl)


def check_mutants(name):
    """every mutant misses the comparison the device passes (check_probe at the GPU tolerances of case `name`) in every loss run; the helper
    without a mutation stays within twice its own record HELPER_DEV
    -> {mutant: smallest factor over the runs by which its worst quantity exceeds the tolerance}"""
    fx = load(name)
    tol = {k: gpu_tol(name, k) for k in CAPS}
    margins = {}
    for tag, r in fx["runs"].items():
        check_probe(mutant_probe(fx, r["loss"], r["C"]), r, {k: 2 * HELPER_DEV[name][k] for k in CAPS}, "%s %s unmutated" % (name, tag))
        for mu in MUTANTS:
            got = mutant_probe(fx, r["loss"], r["C"], mu)
            try:
                check_probe(got, r, tol, "%s %s %s" % (name, tag, mu))
            except AssertionError:
                d = deviations(got, r)
                margins[mu] = min(margins.get(mu, np.inf), max(d[k] / tol[k] for k in d))
            else:
                raise AssertionError("mutant %s passes the probe comparison of case %s, %s" % (mu, name, tag))
    return margins


# ================================================================================================
# self-checks
# ================================================================================================
def ulps(a, b):
    """largest distance of two float64 arrays in units of the last place of the larger magnitude"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    return float((np.abs(a - b) / sp).max()) if a.size else 0.0


def self_check(name, runs=tuple((loss, C) for _, loss, C in LOSS_RUNS)):
    """doubling the digits and dividing the step by 1e5 changes no float64 output by more than 1 ulp -> worst ulps seen"""
    c = case(name)
    W, N = c["obs"].shape[:2]
    worst = 0.0
    lin_a = linearise(c["K"], c["poses0"], c["points0"], c["obs"], DPS, H_STEP)
    lin_b = linearise(c["K"], c["poses0"], c["points0"], c["obs"], 2 * DPS, "1e-30")
    for x, y in zip(jacobians_f64(lin_a, W, N), jacobians_f64(lin_b, W, N)):
        worst = max(worst, ulps(x, y))
    for loss, C in runs:
        sa, sb = system(lin_a, W, N, loss, C, LAM, DPS), system(lin_b, W, N, loss, C, LAM, 2 * DPS)
        for k in PER_LOSS:
            worst = max(worst, ulps(sa[k], sb[k]))
    return worst
