"""The line bench.py prints is the driver's only view of a round: it must be ONE compact strict-JSON object below 4 KB carrying the contract's
keys, `roofline` and `cpu_baseline` -- whatever the full result object holds (the round-5 line grew to 30 KB and was not read)."""
import copy
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                 "config", "roofline", "cpu_baseline")


def _strict_loads(line):
    def no_constants(x):
        raise ValueError("non-finite constant %r in the line" % x)
    return json.loads(line, parse_constant=no_constants)


@pytest.fixture(scope="module")
def canned():
    """a full result object as a default run produced it (round 5: 30 KB, every informational key)"""
    with open(os.path.join(ROOT, "profiles", "r05_bench_default.json")) as f:
        return json.loads(f.read().strip().splitlines()[-1])


def test_compact_line_is_small_strict_and_complete(canned):
    import bench
    line = bench.compact_line(canned, "bench_extras.json")
    assert "\n" not in line and len(line.encode()) < bench.LINE_MAX_BYTES <= 4096
    d = _strict_loads(line)
    for k in CONTRACT_KEYS:
        assert k in d, k
    assert d["value"] == canned["value"] and d["ms_per_step"] == canned["ms_per_step"] and d["steps"] == canned["steps"]
    assert d["config"]["workload"] == "kitti_shaped_1241x376_2000pts_ba10" and "model" not in d["config"]
    assert d["config"]["sequences_per_gpu"] == 256 and d["config"]["ba_lm_iteration_budget"] == 30
    assert d["config"]["stream_layout"] == {"layout": 2, "gate_groups": 4, "reserved_cus": 32} and d["config"]["solves_stopped_by_cap"] == 0
    r = d["roofline"]
    for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us", "algorithmic_bytes_per_launch"):
        assert k in r, k
    assert r["bound"] == "hbm" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4
    assert r["valu"]["frac"] > 0 and r["issue"]["frac_of_quarter_rate_capacity"] > 0
    assert len(r["kernels"]) == 3 and r["kernels"][0]["kernel"].startswith("k_klt_track")
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 16 and c["value"] > 0 and c["unit"] == "frames/s" and c["reference_recipe_ba_seconds_per_adjust"] > 0
    assert d["extras_file"] == "bench_extras.json"
    # the informational keys stay in the side file
    for k in ("pipeline_step", "single_sequence", "klt_only", "dropin_step", "lm_cap_10", "config5_n1"):
        assert k not in d


def test_compact_line_carries_the_second_figures_and_sheds_them_before_the_limit(canned):
    import bench
    full = copy.deepcopy(canned)
    full["host_frames"] = {"value": 44000.0, "unit": "frames/s", "ms_per_step": 5.8, "h2d_gb_s": 20.5}
    full["closed_loop_w10_256"] = {"value": 49871.0, "unit": "frames/s", "ms_per_step": 5.13, "sequences": 256, "capacity_policy_frames": 30720,
                                   "roofline": {"kernel": "k_klt_track", "frac": 0.70}}
    d = _strict_loads(bench.compact_line(full, "bench_extras.json"))
    assert d["host_frames"]["value"] == 44000.0 and d["closed_loop_w10_256"]["value"] == 49871.0
    # a second figure that explodes (say, an error text of 10 KB) is dropped, the contract's keys are not
    full["closed_loop_w10_256"] = {"error": "x" * 10000}
    line = bench.compact_line(full, "bench_extras.json")
    assert len(line.encode()) < bench.LINE_MAX_BYTES
    d = _strict_loads(line)
    assert "closed_loop_w10_256" not in d
    for k in CONTRACT_KEYS:
        assert k in d, k


def test_compact_line_never_prints_a_non_finite_number(canned):
    import bench
    import numpy as np
    full = copy.deepcopy(canned)
    full["roofline"]["traffic"] = float("nan")
    full["roofline"]["valu"]["frac"] = np.float32("inf")
    full["cpu_baseline"]["per_core"] = np.float64("nan")
    full["config"]["solves_note"] = np.int64(3)
    d = _strict_loads(bench.compact_line(full))
    assert d["roofline"]["traffic"] is None and "valu" not in d["roofline"] and "per_core" not in d["cpu_baseline"]


def test_compact_line_of_the_other_workloads():
    """config 5 and the closed loop print through the same function: no roofline.kernels, a null cpu_baseline"""
    import bench
    full = {"metric": "frames/sec, Pipeline.step resident on the device", "value": 49871.0, "unit": "frames/s", "n_gpus": 1, "steps": 40, "warmup": 10,
            "ms_per_step": 5.13, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8/i32 + f64", "data": "synthetic",
            "config": {"workload": "pipeline_step_closed_loop_1241x376_ba10", "sequences_per_gpu": 256, "batched_contexts_per_gpu": 1, "parallelism": "independent sequences"},
            "pipeline": {"big": list(range(5000))}, "roofline": {"bound": "hbm", "kernel": "k_klt_track", "achieved": 5611.3, "peak": 8000.0, "unit": "GB/s", "frac": 0.7014,
                                                                "traffic": None, "avg_launch_us": 2953.6, "algorithmic_bytes_per_launch": 16573466624},
            "cpu_baseline": None}
    line = bench.compact_line(full)
    d = _strict_loads(line)
    assert len(line) < 1500 and d["cpu_baseline"] is None and d["roofline"]["frac"] == 0.7014 and "pipeline" not in d


def _parse(argv, monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_a_plain_run_times_its_steps_once_and_full_restores_the_rest(monkeypatch):
    a = _parse(["--gpus", "1", "--steps", "20", "--warmup", "5"], monkeypatch)
    assert not a.full and a.regions == 1 and a.steps == 20 and a.warmup == 5 and a.dump_outputs is None
    a = _parse(["--full"], monkeypatch)
    assert a.full and a.regions == 5
    a = _parse(["--extras", "--regions", "3"], monkeypatch)
    assert a.full and a.regions == 3


class _FakeCtx:
    def step_layout(self):
        return {"layout": 2, "gate_groups": 4, "reserved_cus": 32}


class _FakeGroup:
    """what bench.Group holds after a fetch: `last` = VoContext.frame_fetch()'s dict for a batch of B sequences"""

    def __init__(self, B, seed, n_pts=2000, n_new=1000, n_lm=2000, W=10):
        import numpy as np
        rng = np.random.default_rng(seed)
        self.B, self.c = B, _FakeCtx()
        self.at_cap = self.truncated = 0
        stats = [dict(cost0=10.0 + b, cost=1.0 + b, lam=1e-3, iters=5 + b % 3, accepted=4, status=2, n_obs=n_lm * W) for b in range(B)]
        corners = [rng.integers(0, 300, (int(rng.integers(0, 20)), 2)).astype(np.float32) for _ in range(B)]
        self.last = dict(points2d=rng.random((B, n_pts, 2), dtype=np.float32), status=rng.integers(0, 2, (B, n_pts)).astype(np.uint8),
                         err=rng.random((B, n_pts), dtype=np.float32), X4=rng.random((B, 4, n_new), dtype=np.float32), depth1=rng.random((B, n_new)),
                         reproj=rng.random((B, n_new)), poses=rng.random((B, W, 6)), landmarks=rng.random((B, n_lm, 3)),
                         ba_stats=stats, corners=corners)
        if B == 1:
            self.last = {k: v[0] for k, v in self.last.items()}          # (VoContext drops the batch axis of a batch of one)

    def ba_stats0(self):
        st = self.last["ba_stats"]
        return st[0] if isinstance(st, list) else st


def test_dump_outputs_writes_the_last_step_as_float_arrays(tmp_path):
    import bench
    import numpy as np
    seqs = [_FakeGroup(3, 1), _FakeGroup(1, 2)]
    # a solve the budget cut, run again by Group.fetch: the caller receives the second solve's poses and landmarks
    seqs[1].last["ba_poses"], seqs[1].last["ba_points"] = seqs[1].last["poses"] + 1.0, seqs[1].last["landmarks"] + 1.0
    bench.dump_outputs(str(tmp_path), seqs)
    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert set(got) == {"sequence", "points2d", "status", "err", "X4", "depth1", "reproj", "poses", "landmarks", "corners", "corners_count"} | \
        {"ba_" + f for f in ("cost0", "cost", "lam", "iters", "accepted", "status", "n_obs")}
    assert all(v.dtype in (np.float32, np.float64) and len(v) == 4 for v in got.values())
    assert np.array_equal(got["sequence"], np.arange(4))
    assert np.array_equal(got["points2d"][:3], seqs[0].last["points2d"]) and np.array_equal(got["points2d"][3], seqs[1].last["points2d"])
    assert np.array_equal(got["status"][:3], seqs[0].last["status"]) and np.array_equal(got["landmarks"][3], seqs[1].last["ba_points"])
    assert np.array_equal(got["poses"][:3], seqs[0].last["poses"]) and np.array_equal(got["poses"][3], seqs[1].last["ba_poses"])
    assert got["ba_iters"].tolist() == [5, 6, 7, 5] and got["ba_cost"].tolist() == [1.0, 2.0, 3.0, 1.0]
    cs = seqs[0].last["corners"] + [seqs[1].last["corners"]]
    for b, c in enumerate(cs):
        n = int(got["corners_count"][b])
        assert n == len(c) and np.array_equal(got["corners"][b, :n], c) and np.isnan(got["corners"][b, n:]).all()


def test_dump_outputs_of_a_large_batch_is_a_fixed_sample_below_64_mb(tmp_path):
    import bench
    import numpy as np
    seqs = [_FakeGroup(640, 3)]                         # ~73 MB of outputs
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), seqs)
    sizes = sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy"))
    assert sizes <= bench.DUMP_MAX_BYTES
    ia, ib = np.load(tmp_path / "a" / "sequence.npy"), np.load(tmp_path / "b" / "sequence.npy")
    assert np.array_equal(ia, ib) and 0 < len(ia) < 640 and np.all(np.diff(ia) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "landmarks.npy"), seqs[0].last["landmarks"][ia.astype(int)])


def test_the_line_of_a_plain_run_carries_the_contract(monkeypatch):
    import bench
    a = _parse(["--steps", "20", "--warmup", "5"], monkeypatch)
    a.ctxs = 1

    class Dist1:
        world = 1
    seqs = [_FakeGroup(256, 4, n_pts=8, n_new=4, n_lm=8)]
    full = bench.headline_result(a, Dist1(), seqs, [0] * 8, [0.1], 0.1, 256 * 20 / 0.1, 256 * 20, 3.0, False, 0, 0)
    d = _strict_loads(bench.compact_line(full))
    for k in CONTRACT_KEYS:
        assert k in d, k
    assert d["steps"] == 20 and d["warmup"] == 5 and d["ms_per_step"] == 5.0 and d["value"] == 51200.0 and d["unit"] == "frames/s"
    assert d["higher_is_better"] is True and d["metric"] == "frames/sec @1241x376, 2000 KLT pts, 10-frame BA window"
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["config"]["ba_lm_iterations_run"] == 5
