"""CPU: the full-contrast cases of tests/range_cases.py are what they claim to be, and the oracle is right on them.

tests/test_gpu_ranges.py compares the tracker and the corner detector with oracle/vo_oracle.c bit for bit on these inputs; that is worth
something only if (1) the oracle itself agrees with a second formulation there, (2) the inputs really carry the integer sums to the top of the
ranges that the kernels' comments argue about -- asserted from the int64 lane model alone, nothing here runs a kernel -- and (3) the ways a
kernel could be wrong there change an output: each mutant of the numpy models is caught by the new cases, and the three range mutants are
invisible to the old suite's seq_small case."""
import numpy as np
import pytest

import klt_seed_model as km
import range_cases as rc
import vo_oracle as o


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want):
    """(p1, status, err, iters) bit for bit"""
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(got[:4], want[:4]))


# ---- 1. the oracle = the second formulation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.IMAGES)
def test_oracle_is_the_numpy_formulation_on_every_case(name):
    for kind in rc.PAIRS:
        for size in rc.KLT_SIZES:
            a, b = rc.pair(name, kind, *size)
            assert same(o.klt(a, b, rc.points(*size), return_iters=True), rc.model(name, kind, size)), (name, kind, size)


@pytest.mark.parametrize("which", [0, 1])
def test_oracle_is_the_numpy_formulation_at_swept_thresholds_and_criteria(which):
    tag, a, b, p0 = rc.sweep_pairs()[which]
    counts = {}
    for thr in rc.THRESHOLDS + rc.own_thresholds(a, b, p0):
        q = o.klt(a, b, p0, minEigThreshold=thr, return_iters=True)
        assert same(q, km.klt_np(a, b, p0, min_eig_thr=thr)), (tag, thr)
        counts[float(thr)] = int(q[1].sum())
    n = len(p0)
    off = counts[-1.0]                                         # no point fails the threshold test
    if tag == "edges":
        assert counts[0.0] == counts[0.03] == off == n and 0 < counts[0.1] < n // 4
    assert counts[np.inf] == 0 and counts[1e3] == 0
    assert [v for k, v in counts.items() if np.isnan(k)] == [off]
    for mc, eps in rc.CRITERIA:
        q = o.klt(a, b, p0, criteria=(3, mc, eps), return_iters=True)
        assert same(q, km.klt_np(a, b, p0, max_count=mc, eps=eps)), (tag, mc, eps)
        if mc <= 0:
            assert q[3].max() <= 0                             # no iteration anywhere
    assert same(o.klt(a, b, p0, criteria=(3, 1000, 0.0), return_iters=True), o.klt(a, b, p0, criteria=(3, 100, 0.0), return_iters=True))


def test_status_flips_exactly_at_a_points_own_min_eig():
    for tag, a, b, p0 in rc.sweep_pairs():
        own = rc.own_thresholds(a, b, p0)
        assert len(own) == 9 and (tag == "checker2" or len(set(map(float, own))) == 9)     # (a periodic pattern has few different values)
        for k in range(0, len(own), 3):
            below, at, above = (o.klt(a, b, p0, minEigThreshold=t)[1] for t in own[k:k + 3])
            assert np.array_equal(below, at) and above.sum() < at.sum(), (tag, k)


# ---- 2. the corner response, bit for bit ---------------------------------------------------------------------------------------------------
def _st_images():
    from vo_mi355x import synthetic as syn
    out = [(n, s, rc.image(n, *s)) for n in rc.IMAGES for s in rc.ST_SIZES]
    out.append(("texture", (311, 94), np.clip(np.rint(syn.make_texture(94, 311, 13)), 0, 255).astype(np.uint8)))   # test_oracle_crosscheck.py
    return out


@pytest.mark.parametrize("block", [31, 15, 3])
def test_corner_response_bit_exact_second_formulation(block):
    for name, size, img in _st_images():
        assert np.array_equal(_bits(o.min_eig(img, block)), _bits(rc.corner_response_f32(img, block))), (name, size)
        assert np.array_equal(_bits(o.harris(img, block, 0.04)), _bits(rc.corner_response_f32(img, block, True, 0.04))), (name, size)
        # the fused kernel's form: differences of a prefix that wraps are the same sums
        assert np.array_equal(rc.window_sums(img, block, "wrap"), rc.window_sums(img, block)), (name, size)


# ---- 3. the inputs reach the ranges: from the int64 model alone -----------------------------------------------------------------------------
U30 = float(1 << 30)


def _all_sums():
    for name, kind, size in rc.tracker_cases():
        p1, st, err, it, sums = rc.model(name, kind, size)
        yield (name, kind, size), st, it, sums


def test_template_sums_reach_the_top_of_their_range():
    best_mix = best_checker = 0.0
    for (name, kind, size), st, it, sums in _all_sums():
        for r in sums:
            if name == "mix":
                best_mix = max(best_mix, r["A11"]["full"] / U30, r["A22"]["full"] / U30)
            if name == "checker2" and st[r["pt"]]:
                best_checker = max(best_checker, r["A11"]["full"] / U30)
    print("largest template sum: mix %.2f x 2^30, checker2 (tracked points) %.2f x 2^30; the bound 961 * 4080^2 is %.2f x 2^30"
          % (best_mix, best_checker, 961 * 4080 ** 2 / U30))
    assert best_mix >= 14.0 and best_checker >= 4.0


def test_mismatch_sums_reach_the_float64_branch_on_tracked_points():
    best = {}
    for (name, kind, size), st, it, sums in _all_sums():
        for r in sums:
            if st[r["pt"]]:
                for b in r["b1"] + r["b2"]:
                    best[name] = max(best.get(name, 0.0), abs(b["full"]) / U30)
    print("largest |mismatch sum| on a tracked point, x 2^30: %s" % {k: round(v, 2) for k, v in best.items()})
    assert best["checker2"] >= 4.0 and max(best.values()) >= 4.0
    # klt_combine leaves the int32 route at |hi| >= 2^14, i.e. |sum| >= 2^30: both signs occur
    signs = {np.sign(b["full"]) for _, st, _, sums in _all_sums() for r in sums for b in r["b1"] + r["b2"] if abs(b["full"]) >= 1 << 30}
    assert signs == {-1, 1}


def test_accumulator_premises_hold_and_how_much_of_them_is_used():
    """the premises of the comments in csrc/vo_klt_lk.h: a quad's sum of A below 2^31 (they say 2^30.01), per-lane |b| below 2^29, a quad's
    |b| below 2^31 (2^30.99); the error sum through wave_sum_i32 fits int32"""
    lane_a = quad_a = lane_b = quad_b = 0
    for _, st, it, sums in _all_sums():
        for r in sums:
            for c in ("A11", "A12", "A22"):
                lane_a = max(lane_a, int(np.abs(r[c]["lane"]).max())); quad_a = max(quad_a, int(np.abs(r[c]["quad"]).max()))
            for b in r["b1"] + r["b2"]:
                lane_b = max(lane_b, int(np.abs(b["lane"]).max())); quad_b = max(quad_b, int(np.abs(b["quad"]).max()))
    print("fraction of the accumulator limits reached: per-lane A %.4f of 2^29, per-quad A %.4f of 2^31, per-lane |b| %.4f of 2^29, "
          "per-quad |b| %.4f of 2^31" % (lane_a / 2 ** 29, quad_a / 2 ** 31, lane_b / 2 ** 29, quad_b / 2 ** 31))
    assert quad_a < 1 << 31 and lane_b < 1 << 29 and quad_b < 1 << 31
    assert lane_a < 1 << 29                                       # (what wave_sum3_wide asks of its callers)
    # ... and the cases go as far as inputs can.  A quad's A is AT its bound 64 * 4080^2.  |b| pairs |diff| = 8160 with |Ix| = 4080 and the sign
    # of Ix only where the template pixel is 0 below a rising or 255 below a falling edge: half the pixels of a two-pixel pattern, half the bound
    assert quad_a == 64 * 4080 ** 2 and lane_a == 16 * 4080 ** 2
    assert quad_b >= 32 * 8160 * 4080 and lane_b >= 8 * 8160 * 4080
    # the error sum (wave_sum_i32): 31 x 31 differences of at most 255 << 5 fit int32, and a tracked point of the inverse pair is AT that maximum
    assert 961 * 8160 < 1 << 31
    p1, st, err, it, _ = rc.model("checker2", "inverse", rc.KLT_SIZES[0])
    assert err[st == 1].max() == np.float32(255.0)


def test_corner_detector_sums_reach_the_top_and_the_prefix_wraps():
    for name in ("vstripes2", "mix"):
        for w, h in rc.ST_SIZES:
            img = rc.image(name, w, h)
            S, V = rc.window_sums(img), rc.column_sums(img)
            top = np.abs(S).max() / 2 ** 31
            pre = int(V[0, :, :256].sum(1).max())
            print("%s %dx%d: largest window sum %.4f x 2^31 (bound %.4f), 256-column prefix of the 31-row sums %.2f x 2^32"
                  % (name, w, h, top, 961 * 1020 ** 2 / 2 ** 31, pre / 2 ** 32))
            assert 0.46 <= top < 1.0
            assert pre > 1 << 32 or (name == "mix" and w == 259)      # (259 // 2 columns of vertical stripes: 0.96 x 2^32)
            assert np.abs(S).max() > 1 << 24                           # the (float) conversions round


def test_both_outcomes_and_a_level_that_runs_out_of_iterations():
    ran_out = False
    for (name, kind, size), st, it, sums in _all_sums():
        ran_out |= bool((it == 30).any())
        if name in rc.ONLY_REJECTED:
            assert st.sum() == 0, (name, kind, size, rc.ONLY_REJECTED[name])
        else:
            assert 0 < st.sum() < len(st), (name, kind, size)
    assert ran_out


# ---- 4. the mutants -------------------------------------------------------------------------------------------------------------------------
def _changed_somewhere(mutant, runs):
    for a, b, p0, kw in runs:
        if not same(km.klt_np(a, b, p0, mutant=mutant, **kw), km.klt_np(a, b, p0, **kw)):
            return True
    return False


def _new_runs(names=("checker2", "mix"), **kw):
    return [rc.pair(n, k, *s) + (rc.points(*s), kw) for n in names for k in rc.PAIRS for s in rc.KLT_SIZES[:1]]


def _old_run(seq_small):
    from vo_mi355x import synthetic as syn
    frames, _ = seq_small                                           # tests/test_gpu_frontend.py::test_klt_small_image_truncated_pyramid
    return [(frames[0], frames[2], syn.grid_points(400, 320, 240, margin=8, seed=3)[::5], {})]


@pytest.mark.parametrize("mutant", ["int32_sums", "int32_combine"])
def test_range_mutants_are_caught_by_the_new_cases_only(mutant, seq_small):
    assert _changed_somewhere(mutant, _new_runs())
    assert not _changed_somewhere(mutant, _old_run(seq_small))


def test_threshold_mutant_is_caught():
    tag, a, b, p0 = rc.sweep_pairs()[0]
    assert _changed_somewhere("thr_le", [(a, b, p0, dict(min_eig_thr=t)) for t in rc.own_thresholds(a, b, p0)[1::3]])


def test_rounding_mutant_is_caught_by_the_tie_lattices():
    runs = _new_runs()
    assert _changed_somewhere("half_up", runs)
    # the template weights of the lattice points alone do it: no iteration, the eigenvalue test off, so only A and status can move
    lattice = [(a, b, p0[rc.N_INT:], dict(max_count=0, min_eig_thr=-1.0)) for a, b, p0, kw in runs]
    tr_a, tr_b = [], []
    a, b, p0, kw = lattice[0]
    km.klt_np(a, b, p0, trace=tr_a, **kw); km.klt_np(a, b, p0, trace=tr_b, mutant="half_up", **kw)
    assert any(not np.array_equal(x["gx"], y["gx"]) or not np.array_equal(x["Iw"], y["Iw"]) for x, y in zip(tr_a, tr_b))


def test_clamp_mutant_is_caught():
    tag, a, b, p0 = rc.sweep_pairs()[0]
    for kw in (dict(eps=-1.0), dict(eps=11.0), dict(max_count=1000, eps=0.0)):
        hit = _changed_somewhere("unclamped", [(a, b, p0, kw)])
        print("unclamped %s: %s" % (kw, "caught" if hit else "same results"))
    assert _changed_somewhere("unclamped", [(a, b, p0, dict(eps=-1.0))])
    assert _changed_somewhere("unclamped", [(a, b, p0, dict(max_count=m, eps=0.0)) for m in (101, 1000)])


def test_saturating_prefix_mutant_is_caught_by_the_new_images_only(seq_small):
    hit = []
    for name, harris in (("mix", False), ("vstripes2", True)):        # (the eigenvalue of `vstripes2` is a - |a| = 0 whatever the sum)
        for w, h in rc.ST_SIZES:
            img = rc.image(name, w, h)
            want = o.harris(img, 31, 0.04) if harris else o.min_eig(img, 31)
            assert np.array_equal(_bits(rc.corner_response_f32(img, 31, harris, 0.04, prefix="wrap")), _bits(want))
            hit.append(not np.array_equal(_bits(rc.corner_response_f32(img, 31, harris, 0.04, prefix="saturate")), _bits(want)))
    assert all(hit)
    old = seq_small[0][1]                                           # tests/test_gpu_frontend.py::test_shi_tomasi_parameter_sweep
    assert np.array_equal(_bits(rc.corner_response_f32(old, 31, prefix="saturate")), _bits(o.min_eig(old, 31)))
