"""CPU-only: the scenario table of tests/ba_lm_cases.py proves itself on the float64 oracle -- every case takes the branch and the exit it is
named for, far enough from every threshold that the device cannot decide otherwise through rounding, and together the cases reach every
branch of `ba_decide` a finite problem can reach with a margin (not: a predicted reduction <= 0, a failed Cholesky of a finite system)."""
import numpy as np
import pytest

import ba_lm_cases as lc

# The device agrees with the oracle to ~1e-7 relative in cost after a whole solve (tests/test_gpu_ba.py): a decision two orders of magnitude further
# from its threshold cannot flip through rounding.  A condition on the inputs: a scene that misses it is replaced, the bar stays.
MARGIN = 1e-5

ALL = lc.CASES + lc.BATCH


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_case_takes_its_exit_with_margin(case):
    r = lc.classify(case)
    ref = r["ref"]
    assert r["exit"] == case["exit"], (r["exit"], r["kinds"])
    assert ref["status"] == lc.STATUS[case["exit"]]
    if "iters" in case:
        assert ref["iters"] == case["iters"]
    assert ref["iters"] <= 30 and ref["points"].shape[0] <= 130
    assert ref["accepted"] == sum(k.startswith("accept") for k in r["kinds"])
    assert r["margin"] >= MARGIN, r["margin"]
    assert r["branch_margin"] >= MARGIN, r["branch_margin"]


@pytest.mark.parametrize("case", lc.FINITE + lc.BATCH, ids=[c["name"] for c in lc.FINITE + lc.BATCH])
def test_case_is_reproducible_on_the_oracle(case):
    """A case can only pin the device where the oracle pins itself: with the points perturbed by 1e-15 relative the oracle takes the same
    decisions, and its cost after every iteration and its final x move by at most a tenth of the bounds the device is held to (cost 1e-7,
    poses 1e-6, points 1e-5).  Like the margin, a condition on the inputs.  (The same scenes with lambda0 = 1e-9 and lambda_min = 1e-12
    miss it by eight orders of magnitude: ba_lm_cases' docstring.)"""
    st = lc.stability(case)
    assert st["same"]
    assert st["cost"] <= 1e-8 and st["poses"] <= 1e-7 and st["points"] <= 1e-6, st


def _kinds(name):
    return lc.classify(lc.BY_NAME[name])["kinds"]


def _runs(kinds):
    """lengths of the runs of consecutive rejections"""
    out, n = [], 0
    for k in kinds + ["end"]:
        if k == "reject":
            n += 1
        elif n:
            out.append(n); n = 0
    return out


def test_rejections_come_in_runs_between_accepts():
    """lambda nu with nu doubling inside a run, nu reset by the accept behind it, and the next linearisation at the old x: runs of up to 5
    rejections, before the first accepted step and behind accepted steps, on every window"""
    runs = {name: _runs(_kinds(name)) for name in ("rejections_w2", "rejections_w4", "rejections_w4b", "rejections_w10", "rejections_w10b", "alternating_w10")}
    assert runs == {"rejections_w2": [2], "rejections_w4": [3, 5], "rejections_w4b": [5, 4], "rejections_w10": [2], "rejections_w10b": [3],
                    "alternating_w10": [1, 2, 2, 2]}
    for name in ("rejections_w4", "rejections_w4b"):      # a run, accepts, another run: nu must restart at 2
        kinds = _kinds(name)
        first, last = kinds.index("reject"), len(kinds) - 1 - kinds[::-1].index("reject")
        assert any(k.startswith("accept") for k in kinds[first:last]) and kinds[-1].startswith("accept"), name
    assert _kinds("rejections_w4")[0] == "reject"               # the first trial of all is rejected: x[cur] is still the seeded x0
    assert _kinds("rejections_w10")[0].startswith("accept")      # a run behind an accepted step: cams[cur ^ 1] holds the trial cameras


def test_every_form_of_the_damping_update_is_reached():
    seen = {}
    for case in lc.FINITE:
        r = lc.classify(case)
        for k, f in zip(r["kinds"], r["factors"]):
            seen.setdefault(k, []).append(f)
    assert set(seen) == {"accept-clamped", "accept-unclamped", "accept-floored", "reject"}
    # an unclamped step that a wrong formula would move far: f >= 1/2 (the clamp is at 1/3)
    assert max(seen["accept-unclamped"]) >= 0.5
    assert len(seen["accept-unclamped"]) >= 6
    # and one far from 1, where 1 - (2 rho - 1)^3 and 1 - (2 rho - 1) differ by a tenth (at rho = 1/2 every odd power gives 1)
    assert max(abs(f - 1.0) for f in seen["accept-unclamped"]) >= 0.5
    assert [k for k in _kinds("alternating_w10") if k == "reject" or k == "accept-unclamped"][:4] == ["accept-unclamped", "reject", "accept-unclamped", "reject"]
    # (1: the rejected step that takes the xtol exit leaves lambda alone)
    assert set(seen["reject"]) == {1.0, 2.0, 4.0, 8.0, 16.0, 32.0} and seen["reject"].count(1.0) == 2


def test_every_exit_is_reached():
    exits = {}
    for case in lc.CASES:
        exits.setdefault(lc.classify(case)["exit"], []).append(lc.classify(case)["ref"]["iters"])
    assert set(exits) == set(lc.STATUS)
    assert 0 in exits["gtol"] and 4 in exits["gtol"]                 # gtol before the first step, and later
    assert set(exits["max_iters"]) >= {1, 3, 4, 5, 8}                # both sides of the host's chunks of four launch groups
    assert sorted(exits["max_iters_reject"]) == [1, 3, 5, 11]
    assert sorted(exits["xtol_reject"]) == [3, 7]


def test_a_cut_on_a_rejected_step_keeps_the_last_accepted_x():
    """every iteration of the first five is rejected: accepted 0, the answer is the input bit for bit, whatever the cut; a cut inside the
    second run of rejections answers with the x of the accepted step before the run"""
    for k in (1, 3, 5):
        case = lc.BY_NAME["cut_on_reject_w4_k%d" % k]
        ref = lc.classify(case)["ref"]
        K, poses0, points0, obs = lc.scene(case)
        assert ref["accepted"] == 0 and ref["iters"] == k and ref["cost"] == ref["cost0"]
        assert np.array_equal(ref["poses"], poses0) and np.array_equal(ref["points"], points0)
        assert ref["lam"] == 1e-5 * 2.0 ** (k * (k + 1) // 2)
    case = lc.BY_NAME["cut_on_reject_w4_k11"]
    assert _kinds(case["name"]) == ["reject"] * 5 + [k for k in _kinds(case["name"])[5:9]] + ["reject"] * 2 and _kinds(case["name"])[8].startswith("accept")
    cut, before = lc.classify(case)["ref"], lc.reference(case, max_iters=9)
    assert cut["accepted"] == before["accepted"] == 4 and cut["cost"] == before["cost"]
    assert np.array_equal(cut["poses"], before["poses"]) and np.array_equal(cut["points"], before["points"])


def test_xtol_after_a_rejection():
    r = lc.classify(lc.BY_NAME["xtol_after_reject_w10"])
    assert [k.split("-")[0] for k in r["kinds"]] == ["accept"] * 6 + ["reject"] and r["ref"]["status"] == 3 and r["ref"]["accepted"] == 6
    r = lc.classify(lc.BY_NAME["xtol_after_reject_w4"])
    assert r["kinds"] == ["reject"] * 3 and r["ref"]["status"] == 3 and r["ref"]["accepted"] == 0


def test_gtol_before_the_first_step():
    for W in (2, 4, 10):
        case = lc.BY_NAME["gtol_at_0_w%d" % W]
        ref = lc.classify(case)["ref"]
        assert (ref["status"], ref["iters"], ref["accepted"], ref["lam"]) == (1, 0, 0, 1e-4) and ref["cost"] == ref["cost0"]


def test_non_finite_problems_overflow_the_damping():
    """a NaN in one pose, or in K: every step is rejected, lambda0 2^(1 + ... + 10) > 1e12 ends the run with status 4"""
    for name in ("nan_pose_w4", "nan_K_w4"):
        r = lc.classify(lc.BY_NAME[name])
        ref = r["ref"]
        assert r["kinds"] == ["reject"] * 10
        assert (ref["status"], ref["iters"], ref["accepted"], ref["lam"]) == (4, 10, 0, 1e-4 * 2.0 ** 55)


def test_mixed_batch_mixes():
    its = [lc.classify(c)["ref"]["iters"] for c in lc.BATCH]
    rej = [lc.classify(c)["kinds"].count("reject") for c in lc.BATCH]
    assert max(its) - min(its) >= 6 and sum(r > 0 for r in rej) >= 2, (its, rej)
    assert all(c["scene"]["n_slots"] == 10 and c["scene"]["n_pts"] == 130 for c in lc.BATCH) and len(lc.BATCH) == 8
    assert all((r > 0) == bool(i & 1) for i, r in enumerate(rej)), rej       # clean and noisy in turn
