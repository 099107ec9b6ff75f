"""GPU: k_dlt (csrc/vo_dlt.hip) against LAPACK's float64 SVD of the matrix it builds, at the degenerate edges the pipeline meets.

The bounds, the scenes and their derivations live in tests/dlt_model.py; tests/test_dlt_model.py shows on the CPU that the C oracle stays
inside them.  Nothing here refers to a Jacobi iteration: optimality (|A x| / |x| against the smallest singular value, every point), direction
(against the last right-singular vector where it is separated), the filter statistics recomputed from the returned point, and bit-for-bit
structure tests (a point's result depends only on its own inputs)."""
import numpy as np
import pytest

import dlt_model as dm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from vo_mi355x import VoContext
    with VoContext(64, 64, max_pts=2048) as c:
        yield c


_CACHE = {}


@pytest.fixture(scope="module")
def case(ctx):
    """name -> scene, LAPACK's SVD and the kernel's outputs (computed once per scene)"""
    def get(name):
        if name not in _CACHE:
            s = dm.scene(name)
            A = dm.system(s["P0"], s["P1"], s["uv0"], s["uv1"])
            sv, v4 = dm.svd(A)
            X4, depth1, reproj = ctx.triangulate(*dm.args(s))
            _CACHE[name] = dict(s=s, A=A, sv=sv, v4=v4, X4=X4, depth1=depth1, reproj=reproj, m=dm.model_stats(s, X4))
        return _CACHE[name]
    yield get
    _CACHE.clear()


@pytest.fixture(scope="module")
def normal2048(ctx):
    s = dm.scene("normal", n=2048)
    return s, ctx.triangulate(*dm.args(s))


@pytest.mark.parametrize("name", dm.SCENES)
def test_optimal_at_every_point(case, name):
    c = case(name)
    ex = dm.residual_excess(c["A"], c["sv"], c["X4"])
    print("k_dlt %s: residual excess max %.3f x 2^-24 s1 (point %d)" % (name, np.nanmax(ex), int(np.nanargmax(ex))))
    assert np.all(ex <= 2.0), np.flatnonzero(~(ex <= 2.0))[:10]


@pytest.mark.parametrize("name", [n for n in dm.SCENES if n != "identical"])
def test_direction(case, name):
    """far_origin: only the points over the gap condition (no count asserted); identical has none"""
    c = case(name)
    ok = dm.gap(c["sv"]) >= dm.GAP_MIN
    sa = dm.sin_angle(c["X4"], c["v4"])
    print("k_dlt %s: smallest gap %.2e, %d points under it, sin max %.3e (%.2f x 2^-24)" %
          (name, dm.gap(c["sv"]).min(), int((~ok).sum()), np.nanmax(sa[ok]), np.nanmax(sa[ok]) / dm.U24))
    if name not in dm.DIRECTION_EXEMPT:
        assert (~ok).sum() == 0
    assert np.all(sa[ok] <= dm.SIN_MAX), np.flatnonzero(ok & ~(sa <= dm.SIN_MAX))[:10]


def test_pure_rotation_is_exact(case):
    X4 = case("pure_rotation")["X4"]
    assert not X4[:3].any() and np.all(np.abs(X4[3]) == 1.0)


@pytest.mark.parametrize("name", dm.SCENES)
def test_depth1_equals_the_model(case, name):
    c = case(name)
    m = c["m"]
    dev = dm.stats_deviation(c["depth1"], m["d"], m["td"])
    print("k_dlt %s: depth1 deviation max %.3g tolerances, %d of %d over, model not finite at %d" %
          (name, np.nanmax(dev), int((~(dev <= 1)).sum()), len(dev), int((~np.isfinite(m["d"])).sum())))
    assert np.all(dev <= 1), np.flatnonzero(~(dev <= 1))[:10]


@pytest.mark.parametrize("name", dm.SCENES)
def test_reproj_equals_the_model(case, name):
    c = case(name)
    m = c["m"]
    dev = dm.stats_deviation(c["reproj"], m["r"], m["tr"])
    print("k_dlt %s: reproj deviation max %.3g tolerances, %d of %d over, largest |difference| %.3g px, model not finite at %d" %
          (name, np.nanmax(dev), int((~(dev <= 1)).sum()), len(dev),
           np.nanmax(np.where(np.isfinite(m["r"]) & np.isfinite(c["reproj"]), np.abs(c["reproj"] - m["r"]), 0)), int((~np.isfinite(m["r"])).sum())))
    assert np.all(dev <= 1), np.flatnonzero(~(dev <= 1))[:10]


@pytest.mark.parametrize("name", dm.SCENES)
def test_filter_equals_the_model(case, name):
    c = case(name)
    differs, near = dm.filter_exceptions(c["depth1"], c["reproj"], c["m"])
    print("k_dlt %s: %d kept, filter differs at %d, %d near a threshold" %
          (name, int(dm.keep(c["depth1"], c["reproj"]).sum()), int(differs.sum()), int(near.sum())))
    assert not (differs & ~near).any(), np.flatnonzero(differs & ~near)[:10]
    assert differs.sum() <= 2


@pytest.mark.parametrize("name", dm.SCENES)
def test_without_statistics_is_bit_identical(ctx, case, name):
    c = case(name)
    X4 = ctx.triangulate(*dm.args(c["s"], stats=False))
    assert dm.bits_equal(X4, c["X4"])


# ---- structure, on the `normal` scene: bit for bit ------------------------------------------------------------------------------------
def _cut(s, idx):
    return dict(s, uv0=np.ascontiguousarray(s["uv0"][idx]), uv1=np.ascontiguousarray(s["uv1"][idx]))


def _same(got, ref, idx=slice(None)):
    return dm.bits_equal(got[0], np.ascontiguousarray(ref[0][:, idx])) and dm.bits_equal(got[1], np.ascontiguousarray(ref[1][idx])) and \
        dm.bits_equal(got[2], np.ascontiguousarray(ref[2][idx]))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 2048])
def test_count_does_not_matter(ctx, normal2048, n):
    s, ref = normal2048
    got = ctx.triangulate(*dm.args(_cut(s, slice(0, n))))
    assert got[0].shape == (4, n) and got[1].shape == (n,) and got[2].shape == (n,)
    assert _same(got, ref, slice(0, n))


def test_permutation_permutes(ctx, normal2048):
    s, ref = normal2048
    perm = np.random.default_rng(5).permutation(2048)
    assert _same(ctx.triangulate(*dm.args(_cut(s, perm))), ref, perm)


def test_batch_of_three_cameras_equals_each_alone(ctx):
    from vo_mi355x import VoContext
    scenes = [dm.scene(name, n=193, seed=dm.SEED + k) for k, name in enumerate(("normal", "behind_and_wide", "far_origin"))]
    with VoContext(64, 64, max_pts=2048, batch=3) as cb:
        got = cb.triangulate(*[np.stack([dm.args(s)[k] for s in scenes]) for k in range(7)])
        X4_only = cb.triangulate(*[np.stack([dm.args(s)[k] for s in scenes]) for k in range(4)])
    assert got[0].shape == (3, 4, 193) and got[1].shape == (3, 193) and got[2].shape == (3, 193)
    assert dm.bits_equal(X4_only, got[0])
    for b, s in enumerate(scenes):
        assert _same([g[b] for g in got], ctx.triangulate(*dm.args(s))), b


def test_resident_path_equals_triangulate(normal2048):
    from vo_mi355x import VoContext
    s, ref = normal2048
    with VoContext(64, 64, max_pts=2048) as c:
        c.dlt_upload(*dm.args(s))
        c.dlt_resident()
        c.dlt_resident()
        assert _same(c.dlt_fetch(), ref)
        c.dlt_upload(*dm.args(_cut(s, slice(300, 400))))
        c.dlt_resident()
        got = c.dlt_fetch()
        assert got[0].shape == (4, 100) and got[1].shape == (100,) and got[2].shape == (100,)
        assert _same(got, ref, slice(300, 400))


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_bad_pixel_pair_stays_in_its_lane(ctx, normal2048, bad):
    """lanes 0, 31 and 63 of the second wave: a whole pair, u0 alone, v1 alone.  The kernel's loop is bounded at 60 sweeps whatever it reads."""
    s, ref = normal2048
    n, lanes = 192, [64, 95, 127]
    t = _cut(s, slice(0, n))
    t["uv0"][64], t["uv1"][64] = bad, bad
    t["uv0"][95, 0] = bad
    t["uv1"][127, 1] = bad
    got = ctx.triangulate(*dm.args(t))                         # raises unless the call returns VO_OK
    clean = np.setdiff1d(np.arange(n), lanes)
    assert _same([got[0][:, clean], got[1][clean], got[2][clean]], ref, clean)
    assert not dm.keep(got[1], got[2])[lanes].any(), (got[0][:, lanes], got[1][lanes], got[2][lanes])
