"""GPU: the factored wave-private bundle-adjustment kernels (csrc/vo_ba_factored.hip: k_ba_build_f / k_ba_update_f), which the rule
(vo_tuning.ba_kernels = 0) runs for windows of 9 and 10 slots at a batch of three problems or more, against the wave-private kernels they
replace there (ba_kernels = 2, the same context) and against oracle/ba_oracle.py.

A batch of 3 (one or two problems take the lane-per-observation kernels), the problems with noise of their own so that they finish in different
iterations and the running-problem compaction deals the workgroups out again; the world frame is turned against the cameras' so that the pose
rotations -- and with them Jr and R, the two factors the new kernels apply once per partial set -- are far from the identity.
Shapes (12 landmarks per wave and chunk, 48 per workgroup round):
  W 10, N 25   the last chunk holds one landmark; visibility 0.8: unobserved slots
  W  9, N 97   the fifth lane of a landmark has no second slot; one landmark in the last chunk of the third round
  W 10, N 101  two workgroup rounds and a ragged tail
A live-landmark count below N (the chunks behind it only seed x[0], the last live chunk is partly filled) reaches the kernels through the closed
loop's tables alone: four sequences of the bench's window-10 closed loop, 2 048 slots of which a few hundred are live, under the rule and under
ba_kernels = 2.
Tolerances: those of tests/test_gpu_ba.py for the probe quantities, those of tests/test_gpu_headline.py for cost and x of a solve."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(10, 25, 0.8), (9, 97, 1.0), (10, 101, 0.9)]
B = 3


def _rvec(R):
    th = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    return th / (2 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


def make_problem(W, N, vis, b):
    """problem b of the batch: its own seed and noise levels; world frame turned by Q (X_w = Q X, R_w = R Q^T: the same residuals)"""
    import ba_oracle as bo
    from vo_mi355x import synthetic as syn
    s = syn.make_ba_scene(n_pts=N, n_slots=W, seed=100 * W + 10 * N + b, visibility=vis, pt_noise=0.15 + 0.25 * b, pose_noise=0.01 + 0.02 * b)
    Q = bo.rodrigues_exp([0.7, -1.1, 0.4])
    poses = s["poses0"].copy()
    for i in range(W):
        poses[i, :3] = _rvec(bo.rodrigues_exp(poses[i, :3]) @ Q.T)
    return dict(K=s["K"], poses0=poses, points0=s["points0"] @ Q.T, obs=s["obs"])


@pytest.fixture(scope="module", params=SHAPES, ids=lambda p: "w%d_n%d" % p[:2])
def runs(request):
    """per shape, ONE context of three problems: probe + solve with the wave-private kernels (ba_kernels = 2), probe + two solves with the rule"""
    from vo_mi355x import VoContext
    W, N, vis = request.param
    pr = [make_problem(W, N, vis, b) for b in range(B)]
    K, poses, points, obs = (np.stack([p[k] for p in pr]) for k in ("K", "poses0", "points0", "obs"))
    if vis < 1.0:
        assert np.isnan(obs).any()
    out = {"problems": pr}
    with VoContext(64, 64, max_pts=64, batch=B) as c:
        prm = c.ba_params(max_iters=30, ftol=1e-3, xtol=1e-3)
        for name, fam in (("wave", 2), ("rule", 0)):
            c.set_tuning(ba_kernels=fam)
            c.ba_upload(K, poses, points, obs)
            out[name + "_probe"] = c.ba_probe(lam=1e-3)
            out[name] = c.ba_adjust(K, poses, points, obs, prm)
        out["rule_again"] = c.ba_adjust(K, poses, points, obs, prm)
    return out


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


PROBE_TOL = {"Hpp": 1e-10, "gp": 1e-10, "Hll": 1e-10, "gl": 1e-10, "S": 1e-8, "rhs": 1e-8, "dposes": 1e-6, "dpoints": 1e-6}


def test_probe_matches_the_wave_private_kernels(runs):
    a, b = runs["rule_probe"], runs["wave_probe"]
    for k, tol in PROBE_TOL.items():
        print(k, rel(a[k], b[k]))
        assert rel(a[k], b[k]) <= tol, (k, rel(a[k], b[k]))
    assert abs(a["cost"] - b["cost"]) <= 1e-9 * max(1.0, b["cost"])
    assert np.abs(a["residual"] - b["residual"]).max() <= 1e-9
    # the rule really ran other kernels: the camera sums and the reduced system are formed in another order (the landmark blocks, formed in
    # pass 1 as before, agree bit for bit) -- were the rule to launch k_ba_build_w after all, everything here would be bitwise equal
    assert not np.array_equal(a["Hpp"], b["Hpp"]) and not np.array_equal(a["S"], b["S"])


def test_probe_matches_the_oracle(runs):
    import ba_oracle as bo
    p = runs["problems"][0]
    a = runs["rule_probe"]
    lam = 1e-3
    ne = bo.normal_equations(p["K"], p["poses0"], p["points0"], p["obs"])
    S, rhs, _, _, _ = bo.schur_system(ne, lam)
    dp, dl, _ = bo.lm_step(ne, lam)
    want = {"Hpp": ne["Hpp"], "gp": ne["gp"], "Hll": ne["Hll"], "gl": ne["gl"], "S": S, "rhs": rhs, "dposes": dp, "dpoints": dl}
    for k, tol in PROBE_TOL.items():
        print(k, rel(a[k], want[k]))
        assert rel(a[k], want[k]) <= tol, (k, rel(a[k], want[k]))
    assert abs(a["cost"] - ne["cost"]) <= 1e-9 * max(1.0, ne["cost"])


def test_solves_take_the_same_lm_path_as_the_wave_private_kernels(runs):
    (po, pt, st), (qo, qt, qs) = runs["rule"], runs["wave"]
    assert [(s["iters"], s["accepted"], s["status"]) for s in st] == [(s["iters"], s["accepted"], s["status"]) for s in qs]
    assert len({s["iters"] for s in st}) > 1                 # the problems finish in different iterations: the tail groups were compacted
    for b in range(B):
        print(b, st[b]["iters"], abs(st[b]["cost"] - qs[b]["cost"]) / qs[b]["cost"], np.abs(po[b] - qo[b]).max(), np.abs(pt[b] - qt[b]).max())
        assert abs(st[b]["cost"] - qs[b]["cost"]) <= 1e-7 * qs[b]["cost"] and abs(st[b]["cost0"] - qs[b]["cost0"]) <= 1e-9 * qs[b]["cost0"]
        assert np.abs(po[b] - qo[b]).max() <= 1e-6 and np.abs(pt[b] - qt[b]).max() <= 1e-5
        assert st[b]["cost"] < st[b]["cost0"]


def test_two_runs_are_bitwise_equal(runs):
    (po, pt, st), (qo, qt, qs) = runs["rule"], runs["rule_again"]
    assert np.array_equal(po, qo) and np.array_equal(pt, qt)
    assert [(s["iters"], s["accepted"], s["status"], s["cost"]) for s in st] == [(s["iters"], s["accepted"], s["status"], s["cost"]) for s in qs]


def test_closed_loop_with_fewer_live_landmarks_than_slots(monkeypatch):
    """the bench's window-10 closed loop (bench.PipeGroup: 2 048-slot tables, no resurrection, LM cap 10 with a fixed budget) over four sequences, six
    steps with three in flight: the adjustments see n_live < N.  The rule against ba_kernels = 2: every integer of every record equal (LM
    iterations, accepted steps, status, list lengths, inliers ...), costs to 1e-7 relative, poses to 1e-6 (tests/test_gpu_headline.py)."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from vo_mi355x import VoContext
    n_steps, Bc, slots = 6, 4, 2048
    scenes = bench.pipe_scenes(2, 12, 4321)
    recs = {}
    boot = VoContext(bench.W_IMG, bench.H_IMG, max_pts=4096, device=0)
    try:
        for name, tune in (("wave", {"ba_kernels": 2}), ("rule", {})):
            monkeypatch.setattr(VoContext, "default_tuning", tune)
            g = bench.PipeGroup(0, scenes, boot, 0, Bc, 10, slots, True, 10, False)
            try:
                out = []
                for _ in range(n_steps):
                    g.enqueue()
                    if g.inflight == 3:
                        g.fetch(); out.append(g.last)
                while g.inflight:
                    g.fetch(); out.append(g.last)
            finally:
                g.c.close()
            recs[name] = out
    finally:
        boot.close()
    assert len(recs["rule"]) == len(recs["wave"]) == n_steps
    differ = False
    for s in range(n_steps):
        for b in range(Bc):
            a, w = recs["rule"][s][b], recs["wave"][s][b]
            assert a["status"] == 0 and 0 < a["ba_landmarks"] < slots and a["ba_iters"] >= 1, (s, b, a)      # adjusted, with n_live < N
            for k, v in w.items():
                if isinstance(v, np.ndarray):
                    assert np.abs(a[k] - v).max() <= 1e-6, (s, b, k, np.abs(a[k] - v).max())
                    differ |= not np.array_equal(a[k], v)
                elif isinstance(v, float):
                    assert abs(a[k] - v) <= 1e-7 * max(1.0, abs(v)), (s, b, k, a[k], v)
                    differ |= a[k] != v
                else:
                    assert a[k] == v, (s, b, k, a[k], v)
    print("ba_landmarks", [[r["ba_landmarks"] for r in step] for step in recs["rule"]], "ba_iters", [[r["ba_iters"] for r in step] for step in recs["rule"]])
    assert differ                                            # (the two runs are not the same kernels: the last bits of some cost or pose differ)
