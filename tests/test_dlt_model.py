"""CPU-only: the bounds of tests/dlt_model.py hold for the C oracle's DLT (oracle/vo_oracle.c) on every scene of the GPU test.

The GPU test (test_gpu_dlt.py) applies the same functions to the HIP kernel; these show that the bounds are not so tight that a correct float64
solver misses them, that the scenes are what their names say (rank, gap, points behind the cameras) and that no point of the chosen seed sits
on a filter threshold.  The oracle returns no statistics, so that bound is exercised on the model's own two evaluations."""
import numpy as np
import pytest

import dlt_model as dm

_CACHE = {}


def _case(name):
    if name not in _CACHE:
        import vo_oracle as o
        s = dm.scene(name)
        A = dm.system(s["P0"], s["P1"], s["uv0"], s["uv1"])
        sv, v4 = dm.svd(A)
        X4 = o.triangulate(s["P0"], s["P1"], s["uv0"], s["uv1"])
        _CACHE[name] = dict(s=s, A=A, sv=sv, v4=v4, X4=X4, m=dm.model_stats(s, X4))
    return _CACHE[name]


def test_system_is_the_stated_matrix():
    s = dm.scene("behind_and_wide", n=7)
    A = dm.system(s["P0"], s["P1"], s["uv0"], s["uv1"])
    assert A.shape == (7, 4, 4) and A.dtype == np.float64
    for i in range(7):
        for view, (P, uv) in enumerate(((s["P0"], s["uv0"]), (s["P1"], s["uv1"]))):
            for k in range(4):
                assert A[i, 2 * view, k] == float(uv[i, 0]) * float(P[2, k]) - float(P[0, k])
                assert A[i, 2 * view + 1, k] == float(uv[i, 1]) * float(P[2, k]) - float(P[1, k])
    sv, v4 = dm.svd(A)
    assert np.all(np.diff(sv, axis=1) <= 0)
    assert np.allclose(np.linalg.norm(np.einsum("nij,nj->ni", A, v4), axis=1), sv[:, 3], rtol=0, atol=1e-12 * sv[:, 0].max())


def test_scenes_are_what_they_claim():
    c = _case("pure_rotation")
    assert not c["s"]["P0"][:, 3].any() and not c["s"]["P1"][:, 3].any()                 # exactly zero fourth columns
    assert not c["A"][:, :, 3].any()
    c = _case("identical")
    assert np.array_equal(c["A"][:, :2], c["A"][:, 2:])                                  # rank 2
    assert (c["sv"][:, 2] <= 1e-12 * c["sv"][:, 0]).all()
    c = _case("far_origin")
    assert np.abs(c["s"]["P0"]).max() > 1e6                                              # what float32 has to carry
    c = _case("behind_and_wide")
    X = c["s"]["X"]
    assert (X[1::2, 2] < 0).all() and (X[0::2, 2] > 0).all()
    for name in dm.SCENES:
        assert len(dm.scene(name)["uv0"]) <= 2000


@pytest.mark.parametrize("name", dm.SCENES)
def test_oracle_is_optimal_at_every_point(name):
    c = _case(name)
    ex = dm.residual_excess(c["A"], c["sv"], c["X4"])
    print("DLT oracle %s: residual excess max %.3f x 2^-24 s1" % (name, ex.max()))
    assert np.all(ex <= 2.0)


@pytest.mark.parametrize("name", [n for n in dm.SCENES if n != "identical"])
def test_oracle_direction(name):
    c = _case(name)
    ok = dm.gap(c["sv"]) >= dm.GAP_MIN
    sa = dm.sin_angle(c["X4"], c["v4"])
    print("DLT oracle %s: smallest gap %.2e, %d points under it, sin max %.3e (%.2f x 2^-24)" %
          (name, dm.gap(c["sv"]).min(), int((~ok).sum()), sa[ok].max(), sa[ok].max() / dm.U24))
    if name not in dm.DIRECTION_EXEMPT:
        assert (~ok).sum() == 0
    assert np.all(sa[ok] <= dm.SIN_MAX)


def test_oracle_pure_rotation_is_exact():
    X4 = _case("pure_rotation")["X4"]
    assert not X4[:3].any() and np.all(np.abs(X4[3]) == 1.0)


@pytest.mark.parametrize("name", dm.SCENES)
def test_statistics_model_and_seed(name):
    c = _case(name)
    s, X4, m = c["s"], c["X4"], c["m"]
    dl, rl = dm.stats_ld(X4, s["uv0"], s["uv1"], s["K"], s["H0"], s["H1"])
    # the two evaluations are not finite at the same points, the tolerance is positive and small where they are
    assert np.array_equal(np.isfinite(m["d"]), np.isfinite(dl)) and np.array_equal(np.isfinite(m["r"]), np.isfinite(rl))
    for v, t in ((m["d"], m["td"]), (m["r"], m["tr"])):
        fin = np.isfinite(v)
        assert np.all(t[fin] > 0) and np.all(t[fin] <= 1e-6 * np.maximum(1.0, np.abs(v[fin]))) and np.all(np.isinf(t[~fin]))
    # the deviation measure: 0 for the model itself, inf / nan where only one side is finite
    assert np.nanmax(dm.stats_deviation(m["d"], m["d"], m["td"])) == 0 and np.nanmax(dm.stats_deviation(m["r"], m["r"], m["tr"])) == 0
    assert not np.all(dm.stats_deviation(np.full_like(m["d"], np.nan), m["d"], m["td"])[np.isfinite(m["d"])] <= 1)
    assert np.all(np.isinf(dm.stats_deviation(np.zeros_like(m["r"]), m["r"], m["tr"])[~np.isfinite(m["r"])]))
    # the seed: no point of the oracle's sits within the tolerance of a filter threshold
    differs, near = dm.filter_exceptions(m["d"], m["r"], m)
    print("DLT model %s: %d kept, %d near a threshold, depth1 not finite %d, reproj not finite %d" %
          (name, int(dm.keep(m["d"], m["r"]).sum()), int(near.sum()), int((~np.isfinite(m["d"])).sum()), int((~np.isfinite(m["r"])).sum())))
    assert differs.sum() == 0 and near.sum() == 0
    if name == "behind_and_wide":
        planted = s["X"] @ s["H1"][2, :3] + s["H1"][2, 3]                                  # camera-1 depth of the planted points
        assert (planted[1::2] < 0).mean() > 0.8 and (np.sign(m["d"]) == np.sign(planted)).mean() > 0.9   # both signs occur and come back
    if name == "pure_rotation":
        assert not m["d"].any() and not np.isfinite(m["r"]).any()                            # X = 0 is camera 0's centre
