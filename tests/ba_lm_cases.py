"""The scenario table of the bundle adjustment's LM loop and its classifier.  TEST INFRASTRUCTURE (no test in this module).

`ba_decide` (csrc/vo_ba.hip) takes the only data-dependent branches of the product: accept / reject, the three forms of the damping update, and
five exits.  Every case below is a tiny problem (N <= 130, <= 30 oracle iterations) named for the branch or exit it reaches on the float64
oracle (oracle/ba_oracle.py: `solve` is the same statements as `ba_decide`).  tests/test_ba_lm_cases.py proves on the CPU that each case reaches what it
is named for, at a distance from every threshold that rounding cannot bridge; tests/test_gpu_ba_lm.py then holds the device to the table.

Rejected steps come from a damping that starts two orders of magnitude below its floor (lambda0 = 1e-5, lambda_min = 1e-3) on scenes with
large point noise: the Gauss-Newton step overshoots, for reasons a float64 solver reproduces.  A damping of 1e-9 .. 1e-12 reaches the same
branches but pins nothing: the reduced camera system then has a condition number of 1e12 (the window has 7 gauge freedoms, held by the damping
alone), and the ORACLE's own run changes with the last bit of its input -- a relative perturbation of 1e-15 of the points moves the cost after
the first step of the 2-slot scene from 4193.66 to 3304.50 or turns the accepted step into a rejected one.  `stability` measures exactly that,
and every case here has to pass it.

A case is dict(name, scene, params, exit[, iters][, poison]):
  scene   keyword arguments of synthetic.make_ba_scene
  params  keyword arguments of VoContext.ba_params (oracle_kwargs() renames them for ba_oracle.solve)
  exit    'gtol' | 'ftol' | 'xtol_accept' | 'xtol_reject' | 'max_iters' | 'max_iters_reject' | 'overflow'
  poison  'pose': one pose component NaN; 'K': the whole calibration matrix NaN (the non-finite problems)
"""
import functools

import numpy as np

import ba_oracle as bo
from vo_mi355x import synthetic as syn

STATUS = {"max_iters": 0, "max_iters_reject": 0, "gtol": 1, "ftol": 2, "xtol_accept": 3, "xtol_reject": 3, "overflow": 4}
DEFAULTS = dict(max_iters=50, ftol=1e-3, xtol=1e-3, gtol=1e-8, lambda0=1e-4, lambda_min=1e-3)   # VoContext.ba_params
SIZES = {2: 40, 4: 70, 10: 130, 20: 130}       # window -> landmarks
LOW = dict(lambda0=1e-5, max_iters=30)     # damping far below what the noisy scenes need (and below its floor): their first steps are rejected


def clean(W, seed=None):
    return dict(n_pts=SIZES[W], n_slots=W, seed=40 + W if seed is None else seed, visibility=0.85)


def noisy(W, seed, pt_noise=3.0, pose_noise=0.02, visibility=0.7):
    return dict(n_pts=SIZES[W], n_slots=W, seed=seed, visibility=visibility, pt_noise=pt_noise, obs_noise=1.0, pose_noise=pose_noise)


NOISY_W2 = noisy(2, 109, visibility=1.0)      # RR A...                          (never leaves: cut at 12)
NOISY_W4 = noisy(4, 54)                       # RRR AAAA RRRRR AAAAAA            xtol behind an accepted step
NOISY_W4B = noisy(4, 74, 5.0, 0.05)           # RRRRR AAAA RRRR AAA...           (never leaves: cut at 16)
NOISY_W10 = noisy(10, 86)                     # A RR AAAAAAAAAAAAA               ftol; five unclamped accepts
NOISY_W10B = noisy(10, 108)                   # A RRR AAAAAAAA                   ftol
NOISY_W10C = noisy(10, 82)                    # AAAAAA R                         with ftol = 0, xtol = 0.0259: xtol on the rejected step


# gtol between max |g| after 3 and after 4 iterations of the clean scene (their geometric mean, with ftol = xtol = 0)
GTOL_MID = {2: 1.2396623196147052, 4: 2.897690420942309, 10: 7.170194062424593}

CASES = []


def _case(name, scene, params, exit, **more):
    CASES.append(dict(name=name, scene=scene, params=params, exit=exit, **more))


for _W in (2, 4, 10):
    _case("gtol_at_0_w%d" % _W, clean(_W), dict(gtol=1e9), "gtol", iters=0)
    _case("gtol_at_4_w%d" % _W, clean(_W), dict(ftol=0.0, xtol=0.0, gtol=GTOL_MID[_W]), "gtol", iters=4)
_case("xtol_after_accept_w4", clean(4), dict(ftol=0.0, xtol=1e-3), "xtol_accept", iters=25)
_case("xtol_after_accept_w10", clean(10), dict(ftol=0.0, xtol=1e-3), "xtol_accept", iters=5)
_case("xtol_after_accept_w20", clean(20, seed=60), dict(), "xtol_accept", iters=4)        # the n > 64 back substitution of k_ba_solve
_case("ftol_floored_w4", clean(4), dict(), "ftol", iters=10)                              # lambda0 < lambda_min: every accept lands on the floor
_case("ftol_floored_w10", clean(10), dict(), "ftol", iters=4)
_case("rejections_w2", NOISY_W2, dict(LOW, max_iters=12), "max_iters", iters=12)
_case("rejections_w4", NOISY_W4, dict(LOW), "xtol_accept", iters=18)
_case("rejections_w4b", NOISY_W4B, dict(LOW, max_iters=16), "max_iters", iters=16)
_case("rejections_w10", NOISY_W10, dict(LOW), "ftol", iters=16)
_case("rejections_w10b", NOISY_W10B, dict(LOW), "ftol", iters=12)
# lambda0 = lambda_min = 1e-4: the damping moves freely above its floor, accepted steps take the unclamped gain factor
_case("unclamped_w4", noisy(4, 54, 5.0, 0.05), dict(lambda0=1e-4, lambda_min=1e-4, max_iters=30), "ftol", iters=22)
_case("alternating_w10", noisy(10, 80), dict(lambda0=1e-4, lambda_min=1e-4, max_iters=30), "xtol_accept", iters=17)     # R, RR, RR, RR between accepts
_case("xtol_after_reject_w10", NOISY_W10C, dict(LOW, ftol=0.0, xtol=0.0259), "xtol_reject", iters=7)      # behind six accepted steps
_case("xtol_after_reject_w4", NOISY_W4, dict(LOW, ftol=0.0, xtol=0.365), "xtol_reject", iters=3)           # nothing accepted yet
for _k in (1, 3, 5, 11):     # 1, 3, 5: nothing accepted yet; 11: inside the second run of rejections, four accepted steps before it
    _case("cut_on_reject_w4_k%d" % _k, NOISY_W4B, dict(LOW, max_iters=_k), "max_iters_reject", iters=_k)
for _k in (1, 3, 4, 5, 8):      # both sides of the host's chunks of 4 launch groups
    _case("max_iters_w4_k%d" % _k, clean(4), dict(ftol=0.0, xtol=0.0, gtol=0.0, max_iters=_k), "max_iters", iters=_k)
_case("nan_pose_w4", clean(4), dict(max_iters=20), "overflow", iters=10, poison="pose")
_case("nan_K_w4", clean(4), dict(max_iters=20), "overflow", iters=10, poison="K")

BY_NAME = {c["name"]: c for c in CASES}
FINITE = [c for c in CASES if "poison" not in c]

# the mixed batch (W = 10, N = 130, default parameters but for lambda0): clean and noisy scenes in turn; on the oracle they take
# 4, 16, 4, 12, 4, 16, 4 and 12 iterations, every noisy one with a run of two or three rejected steps
BATCH_PARAMS = dict(lambda0=1e-5)
BATCH = [dict(name="batch%d_%s%d" % (i, "noisy" if i & 1 else "clean", sc["seed"]), scene=sc, params=dict(BATCH_PARAMS), exit="ftol")
         for i, sc in enumerate([clean(10, 41), NOISY_W10, clean(10, 45), noisy(10, 88, 5.0, 0.05), clean(10, 46), NOISY_W10C, clean(10, 51), NOISY_W10B])]


def full_params(case):
    return dict(DEFAULTS, **case["params"])


def oracle_kwargs(params):
    """ba_params' names -> ba_oracle.solve's"""
    p = dict(DEFAULTS, **params)
    return dict(max_iters=p["max_iters"], ftol=p["ftol"], xtol=p["xtol"], gtol=p["gtol"], lam0=p["lambda0"], lam_min=p["lambda_min"])


@functools.lru_cache(maxsize=None)
def _scene(name):
    case = BY_NAME.get(name) or {c["name"]: c for c in BATCH}[name]
    s = syn.make_ba_scene(**case["scene"])
    if case.get("poison") == "pose":
        s["poses0"][1, 4] = np.nan
    elif case.get("poison") == "K":
        s["K"][:] = np.nan
    for v in s.values():
        v.setflags(write=False)
    return s


def scene(case):
    """K, poses0, points0, obs of a case (read-only arrays, built once)"""
    s = _scene(case["name"])
    return s["K"], s["poses0"], s["points0"], s["obs"]


def reference(case, max_iters=None):
    """ba_oracle.solve of the case, optionally cut at max_iters"""
    kw = oracle_kwargs(case["params"])
    if max_iters is not None:
        kw["max_iters"] = max_iters
    return bo.solve(*scene(case), **kw)


@functools.lru_cache(maxsize=None)
def _classify(name):
    case = BY_NAME.get(name) or {c["name"]: c for c in BATCH}[name]
    kw = oracle_kwargs(case["params"])
    args = scene(case)
    trace = []
    ref = bo.solve(*args, trace=trace, **kw)
    margin = bo.loss_solve(*args, **kw)["margin"]
    lam_min = kw["lam_min"]
    lams = ([t["lam"] for t in trace[1:]] + [ref["lam"]])[:len(trace)]        # lambda after iteration 1 .. T
    assert len(lams) == len(trace) == ref["iters"]
    kinds, factors, branch = [], [], np.inf
    rel = lambda a, b: abs(a - b) / abs(b)
    for t, lam_after in zip(trace, lams):
        if t["Ft"] < t["F"] and t["rho"] > 0:
            f = 1.0 - (2.0 * t["rho"] - 1.0) ** 3
            raw = t["lam"] * max(1.0 / 3.0, f)
            branch = min(branch, rel(f, 1.0 / 3.0), rel(raw, lam_min))
            kinds.append("accept-floored" if lam_after == lam_min else "accept-clamped" if f < 1.0 / 3.0 else "accept-unclamped")
            factors.append(f)
        else:
            branch = min(branch, rel(lam_after, 1e12))
            kinds.append("reject")
            factors.append(lam_after / t["lam"])
    last = kinds[-1] if kinds else None
    if ref["status"] == 1:
        ex = "gtol"
    elif ref["status"] == 2:
        ex = "ftol"
    elif ref["status"] == 3:
        ex = "xtol_reject" if last == "reject" else "xtol_accept"
    elif ref["status"] == 4:
        ex = "overflow"
    else:
        ex = "max_iters_reject" if last == "reject" else "max_iters"
    return dict(kinds=kinds, exit=ex, lams=lams, factors=factors, margin=margin, branch_margin=branch, ref=ref)


def classify(case):
    """What the oracle does with the case.  -> dict(
    kinds   per iteration 'accept-clamped' (gain factor 1 - (2 rho - 1)^3 below 1/3) | 'accept-unclamped' | 'accept-floored' (lambda landed on
            lambda_min) | 'reject',
    exit    the exit taken (see the module docstring),
    lams    the oracle's lambda after every iteration,
    factors per iteration the unclamped gain factor of an accept, lambda_k / lambda_k-1 (= nu) of a rejection,
    margin  loss_solve's: the smallest relative distance of an accept / ftol / xtol / gtol decision to its threshold,
    branch_margin  the same for the choices `margin` leaves out: gain factor against 1/3, lambda against lambda_min and against 1e12,
    ref     ba_oracle.solve's result)"""
    return _classify(case["name"])


@functools.lru_cache(maxsize=None)
def _stability(name):
    case = BY_NAME.get(name) or {c["name"]: c for c in BATCH}[name]
    kw = oracle_kwargs(case["params"])
    K, poses0, points0, obs = scene(case)
    base = classify(case)
    trace = []
    ref = bo.solve(K, poses0, points0, obs, trace=trace, **kw)
    rng = np.random.default_rng(1)
    out = dict(same=True, cost=0.0, poses=0.0, points=0.0)
    for _ in range(2):
        tr2 = []
        r2 = bo.solve(K, poses0, points0 * (1.0 + 1e-15 * rng.standard_normal(points0.shape)), obs, trace=tr2, **kw)
        kinds2 = ["accept" if t["Ft"] < t["F"] and t["rho"] > 0 else "reject" for t in tr2]
        if kinds2 != [k.split("-")[0] for k in base["kinds"]] or r2["status"] != ref["status"]:
            out["same"] = False
            continue
        costs = [abs(a["F"] - b["F"]) / a["F"] for a, b in zip(trace, tr2)] + [abs(ref["cost"] - r2["cost"]) / ref["cost"]]
        out["cost"] = max(out["cost"], max(costs))
        out["poses"] = max(out["poses"], np.abs(ref["poses"] - r2["poses"]).max())
        out["points"] = max(out["points"], np.abs(ref["points"] - r2["points"]).max())
    return out


def stability(case):
    """The oracle's own reproducibility on a finite case: two runs with the points perturbed by 1e-15 relative (a few units in the last place).
    -> dict(same: every step accepted / rejected as before and the same exit, cost: the largest relative change of the cost after any
    iteration, poses / points: the largest change of the final x)"""
    return _stability(case["name"])
