"""GPU: every exit and boundary of the depth filter (vo_depth_update, csrc/vo_depth.hip) reached at least once and asserted by code, on the
constructed problems of depth_model.edge_cases() (tests/test_depth_model.py shows that the model reaches each of them and which seeds it
decides alone).  The kernel is compared with the model on every decided seed and on the seeds a case declares exact (A == B: no
perturbation leaves n_steps = 0 as it is, but the kernel's float64 expressions are the model's)."""
import numpy as np
import pytest

import depth_model as dm
from test_gpu_depth import Stores, raw_update, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stores():
    s = Stores()
    yield s
    s.close()


@pytest.mark.parametrize("case", dm.edge_cases(), ids=lambda c: c["name"])
def test_every_exit_and_boundary(stores, case):
    labels = case["labels"]
    extra = np.array([l in case.get("exact", ()) for l in labels])
    (seeds, res, match, z, stats), = run_case(stores.get(case["size"]), case, rows_extra=extra)
    m64 = dm.case_runs(case)[0]["m64"]
    before = dm.case_data(case)["seeds"]
    for i, l in enumerate(labels):
        e = case["expect"].get(l)
        if e is None:
            continue
        assert res[i] == e["code"], (l, dm.NAMES[res[i]])
        if e["code"] >= dm.SKIP_INVISIBLE:
            # a skip leaves the state bit for bit, and reports no depth
            assert seeds[i].tobytes() == before[i].tobytes(), l
            assert np.isnan(z[i]), l
        if e["code"] in (dm.OUTLIER_NOMATCH, dm.OUTLIER_ALIGN):
            assert seeds["b"][i] == before["b"][i] + 1.0 and seeds["mu"][i].tobytes() == before["mu"][i].tobytes(), l
            assert (seeds["flags"][i] >> dm.OBS_SHIFT) == (before["flags"][i] >> dm.OBS_SHIFT) + 1, l
        if e["code"] == dm.UPDATED:
            assert np.isfinite(z[i]) and seeds["sigma2"][i] < before["sigma2"][i], l
        if e.get("left"):
            assert match[i, 0] >= dm.W - 4.0, (l, match[i])                    # the alignment's last centre is past the image's interior
    if case["name"] == "edges":
        # the exact shift of 50 pixels: an updated seed that saw it measures the inverse depth 0.5 (mu is the inverse distance)
        for l in ("steps2", "steps64", "steps65", "steps128", "half_outside"):
            i = labels.index(l)
            fz = dm.bearing(dm.K_E, np.array([[before["u"][i], before["v"][i]]], np.float64))[0, 2]
            assert abs(1.0 / z[i] / fz - 0.5) < 1e-3, (l, z[i])
        assert stats[dm.SKIP_INACTIVE] == sum(1 for l in labels if case["expect"].get(l, {}).get("code") == dm.SKIP_INACTIVE)
    if case["name"] == "tie":
        assert m64["tied"].all() and np.array_equal(np.round(match).astype(np.int64), m64["best_px"])


def test_seed_counts_at_the_wave_and_chunk_edges(stores):
    """n = 0, 1, 63, 64, 65 and 257 seeds: every seed is a wave of its own, four to a workgroup; a call on the first n rows gives those rows
    of the full call bit for bit, touches no row behind them and counts n results"""
    (case,) = [c for c in dm.gpu_cases() if c["name"] == "n257_edges"]
    d = dm.case_data(case)
    ctx = stores.get(case["size"])
    img, poses = d["steps"][0]
    ctx.push_frame(img)
    full = d["seeds"].copy()
    want = raw_update(ctx, d["K"], poses, full, d["patches"])
    assert want[0] == 0 and want[4][0][:7].sum() == 257
    st = dm.case_runs(case)[0]
    dec = st["decided"]
    assert np.array_equal(want[1][0][dec], st["m64"]["result"][dec])
    for n in (0, 1, 63, 64, 65, 257):
        s = d["seeds"].copy()
        got = raw_update(ctx, d["K"], poses, s, d["patches"], n=n)
        assert got[0] == 0 and got[4][0][:7].sum() == n
        assert s[:n].tobytes() == full[:n].tobytes() and s[n:].tobytes() == d["seeds"][n:].tobytes()
        assert all(got[k][0][:n].tobytes() == want[k][0][:n].tobytes() for k in (1, 2, 3))
        assert (got[1][0][n:] == 255).all() and (got[2][0][n:] == -1.0).all() and (got[3][0][n:] == -1.0).all()


def test_a_bad_seed_leaves_its_neighbours_as_they_are(stores):
    """the good seeds of the edge case, updated alone, come out bit for bit as they do between the bad ones"""
    (case,) = [c for c in dm.edge_cases() if c["name"] == "edges"]
    d = dm.case_data(case)
    ctx = stores.get(case["size"])
    img, poses = d["steps"][0]
    ctx.push_frame(img)
    mixed = d["seeds"].copy()
    a = raw_update(ctx, d["K"], poses, mixed, d["patches"])
    rows = np.array([l.startswith("good_after") for l in case["labels"]])
    assert rows.sum() >= 20
    alone = np.ascontiguousarray(d["seeds"][rows])
    b = raw_update(ctx, d["K"], poses, alone, np.ascontiguousarray(d["patches"][rows]))
    assert a[0] == b[0] == 0 and (b[1][0] == dm.UPDATED).all()
    assert alone.tobytes() == np.ascontiguousarray(mixed[rows]).tobytes()
    assert all(np.ascontiguousarray(a[k][0][rows]).tobytes() == b[k][0].tobytes() for k in (1, 2, 3))
