"""CPU-only: the model of sparse direct image alignment (tests/align_model.py) against itself and against ground truth -- its Jacobian
against finite differences, the pose it finds on rendered frames with known motion, its parameters and degenerate rows, and the condition on
the inputs of tests/test_gpu_align.py: which of them the model alone decides.  For the edge cases of tests/test_gpu_align_edges.py: that the
model decides them (by margin, or by a declared structural zero), that they reach every exit and level shape they are named for, that the
border an unused point samples does not matter, and the Rodrigues / log round trip that bounds the log_exp cases.  Every figure is printed
before it is asserted."""
import numpy as np
import pytest

import align_model as am


def _E(xi):
    return am.rodrigues(xi[3:]), np.asarray(xi[:3], np.float64)


def test_geometric_jacobian_against_finite_differences():
    rng = np.random.default_rng(5)
    K = np.array([[400.0, 0, 103.5], [0, 380.0, 59.5], [0, 0, 1]])
    X = np.stack([rng.uniform(-2, 2, 20), rng.uniform(-1, 1, 20), rng.uniform(4, 12, 20)], 1)
    worst = 0.0
    for l in (0, 1):
        J = am.jacobian(K, l, X)
        for k in range(6):
            h = 1e-6
            xi = np.zeros(6); xi[k] = h
            Rp, vp = _E(xi); Rm, vm = _E(-xi)
            fd = (am.project(K, l, X @ Rp.T + vp) - am.project(K, l, X @ Rm.T + vm)) / (2 * h)
            worst = max(worst, np.abs(fd - J[:, :, k]).max() / max(np.abs(J[:, :, k]).max(), 1.0))
    print("J_p against central differences of pi_l(E(xi) X): worst relative difference %.3g" % worst)
    # central differences at h = 1e-6 on coordinates of a few hundred pixels: truncation h^2, rounding 1e-16 x 400 / 1e-6 = 4e-8
    assert worst <= 1e-6


def test_photometric_jacobian_against_finite_differences_of_the_models_own_residual():
    # on an image that is linear in x and y bilinear sampling and central differences are exact, so the residual's derivative is -g J_p
    ys, xs = np.mgrid[0:60, 0:104].astype(np.float64)
    prev = 20.0 + 0.75 * xs + 1.5 * ys
    cur = prev + 3.0
    K = np.array([[200.0, 0, 51.75], [0, 190.0, 29.75], [0, 0, 1]])
    rng = np.random.default_rng(9)
    X = np.stack([rng.uniform(-1.0, 1.0, 12), rng.uniform(-0.5, 0.5, 12), rng.uniform(5, 9, 12)], 1)
    ref = am.reference(prev, K, 0, X)
    assert ref["ok"].all() and np.allclose(ref["gx"], 0.75) and np.allclose(ref["gy"], 1.5)
    lin = am.linearise(ref, cur, K, 0, np.eye(3), np.zeros(3), 0.0)
    assert np.allclose(lin["res"], 3.0) and lin["n_used"] == 12
    worst = 0.0
    for k in range(6):
        h = 1e-6
        xi = np.zeros(6); xi[k] = h
        r = []
        for s in (1, -1):
            R, v = _E(s * xi)
            moved = am.reference(prev, K, 0, X @ R.T + v)            # I_prev(pi(E(xi) X) + o)
            r.append(lin["res"] + ref["I"] - moved["I"])
        fd = (r[0] - r[1]) / (2 * h)                                # d r / d xi_k per pixel
        an = -(ref["gx"] * ref["J"][:, 0, k][:, None] + ref["gy"] * ref["J"][:, 1, k][:, None])
        worst = max(worst, np.abs(fd - an).max() / max(np.abs(an).max(), 1.0))
    print("-(gx J_p[0] + gy J_p[1]) against central differences of the residual: worst relative difference %.3g" % worst)
    assert worst <= 1e-5
    # and the normal equations are what those Jacobians sum to
    Jpix = ref["gx"][:, :, None] * ref["J"][:, None, 0, :] + ref["gy"][:, :, None] * ref["J"][:, None, 1, :]
    assert np.allclose(lin["H"], np.einsum("npi,npj->ij", Jpix, Jpix), rtol=1e-12) and np.allclose(lin["b"], np.einsum("npi,np->i", Jpix, lin["res"]), rtol=1e-12)


@pytest.mark.parametrize("n", [64, 128])
def test_pose_on_rendered_frames_is_within_a_tenth_of_the_image_motion(n):
    sc = am.scene(am.W, am.H)
    for seed in range(4):
        t = seed
        X = am.scene_points(sc, t, n, seed)
        P, C = am.pyramid(sc["frames"][t], am.LEVELS), am.pyramid(sc["frames"][t + 1], am.LEVELS)
        m = am.run(P, C, sc["K"], X, huber=10.0)
        motion, err = am.prediction_error(sc["K"], X, m["R"], m["t"], *am.true_pose(sc, t))
        print("n %d seed %d pair %d: median image motion %.3f px, median prediction error %.4f px (1/%.0f), iters %s, chi %.2f"
              % (n, seed, t, motion, err, motion / err, m["iters"][:2], m["chi2"]))
        assert m["status"] == 0 and m["levels_run"] == 2 and err <= motion / 10.0


def _case(name):
    (c,) = [c for c in am.gpu_cases() if c["name"] == name]
    return c, am.case_runs(c)[0]


def test_parameters_behave_as_specified():
    sc = am.scene(am.W, am.H)
    c, m = _case("huber0")
    P, C = am.pyramid(sc["frames"][c["t"]], am.LEVELS), am.pyramid(sc["frames"][c["t"] + 1], am.LEVELS)
    ref = am.reference(P[0], c["K"], 0, c["X"].astype(np.float64))
    l0, l10 = am.linearise(ref, C[0], c["K"], 0, np.eye(3), np.zeros(3), 0.0), am.linearise(ref, C[0], c["K"], 0, np.eye(3), np.zeros(3), 10.0)
    big = np.abs(l0["res"]) > 10.0
    assert (l0["w"] == 1.0).all() and big.any() and np.allclose(l10["w"][big], 10.0 / np.abs(l10["res"][big])) and (l10["w"][~big] == 1.0).all()
    assert l10["chi"] < l0["chi"]
    c, m = _case("min_level1")
    assert m["iters"][0] == 0 and m["iters"][1] > 0 and m["levels_run"] == 1
    c, m = _case("max_iters1")
    assert list(m["iters"][:2]) == [1, 1] and m["levels_run"] == 2
    # an initial pose: starting at the truth the first linearisation of the top level already has the small residual, and the result stays there
    c, m = _case("n64")
    Rt, tt = am.true_pose(sc, c["t"])
    P, C = am.pyramid(sc["frames"][c["t"]], am.LEVELS), am.pyramid(sc["frames"][c["t"] + 1], am.LEVELS)
    m2 = am.run(P, C, c["K"], c["X"], am.log_so3(Rt), tt)
    d = am.displacement(c["K"], c["X"], m2["R"], m2["t"], Rt, tt)
    print("started at the truth: ends %.3f px from it (largest displacement), from identity %.3f px" % (d, am.displacement(c["K"], c["X"], m["R"], m["t"], Rt, tt)))
    assert d <= 1.0 and m2["status"] == 0
    c, m = _case("init_pose")
    assert m["status"] == 0 and m["levels_run"] == 2


def test_degenerate_rows_and_too_few_points():
    c, m = _case("nan_and_behind")
    X = c["X"]
    bad = ~(np.isfinite(X).all(1) & (X[:, 2] > 0))
    print("nan_and_behind: %d of %d rows are NaN or not in front; used %d" % (bad.sum(), len(X), m["n_used"]))
    assert bad.sum() == 17 and not m["used"][bad].any() and m["n_used"] == int(m["used"].sum()) == len(X) - 17 and m["status"] == 0
    # the same rows alone give the same pose: the bad rows contribute nothing
    sc = am.scene(am.W, am.H)
    P, C = am.pyramid(sc["frames"][c["t"]], am.LEVELS), am.pyramid(sc["frames"][c["t"] + 1], am.LEVELS)
    m2 = am.run(P, C, c["K"], X[~bad])
    assert am.displacement(c["K"], X, m["R"], m["t"], m2["R"], m2["t"]) <= 1e-9
    c, m = _case("n9")
    assert m["status"] == am.VO_E_NUMERIC and list(m["iters"][:2]) == [-1, -1] and m["levels_run"] == 0 and not m["used"].any()
    assert np.array_equal(m["rvec"], c["rvec0"]) and np.array_equal(m["tvec"], c["tvec0"])
    # points that leave the interior while the level iterates: the count of used points changes from one pass to a later one
    for name in ("leaving", "leaving_n200"):
        c, m = _case(name)
        counts = [v for k, v, _ in m["margins"] if k == "min_points"]
        print(name, "used per pass:", counts)
        assert len(set(counts)) > 1 and m["n_used"] < len(c["X"])


def test_the_gpu_tests_inputs_are_decided_by_the_model_alone():
    cases = am.gpu_cases()
    dec = []
    for c in cases:
        a, b = am.case_runs(c)
        dec.append(am.decided(a, b))
        print("%-16s n %3d iters %s n_used %3d decided %s; float32 switch moves the pose by %.3g px"
              % (c["name"], len(c["X"]), a["iters"][:2], a["n_used"], dec[-1], am.displacement(c["K"], c["X"], a["R"], a["t"], b["R"], b["t"])))
    assert {len(c["X"]) for c in cases} >= {9, 10, 17, 64, 200}
    assert sum(dec) >= 0.8 * len(cases), dec


# ---- the edge cases of tests/test_gpu_align_edges.py ------------------------------------------------------------------------------------
def _edge(name):
    (c,) = [c for c in am.edge_cases() + am.mixed_batch() if c["name"] == name]
    return c, am.case_runs(c)[0]


def _ends(m, levels):
    return [am.END_NAMES[int(e)] for e in m["ends"][:levels]]


def test_the_edge_cases_are_decided_by_the_model_alone():
    """a condition on the inputs, not a measurement: every stop decision of a case is either clear of its threshold by 4 x what the float32
    switch moves it, or a structural zero the case declares -- and then its value IS the threshold in the float64 and in the float32 run"""
    cases = am.edge_cases() + am.mixed_batch()
    dec = []
    for c in cases:
        a, b = am.case_runs(c)
        lv = am.case_store(c)[2]
        dec.append(am.case_decided(c))
        print("%-26s %3dx%-3d n %3d iters %-16s ends %-42s flags %-9s n_used %3d decided %s%s; float32 switch moves the pose by %.3g px"
              % (c["name"], c["size"][0], c["size"][1], len(c["X"]), a["iters"][:lv], _ends(a, lv), am.END_NAMES[a["flags"]], a["n_used"], dec[-1],
                 " (exact: %s)" % ", ".join(c["exact"]) if c["exact"] else "", am.displacement(c["K"], c["X"], a["R"], a["t"], b["R"], b["t"])))
        if c["exact"]:
            for m in (a, b):
                ex = am.exact_margins(m, c["exact"])
                assert ex and {k for k, _, _ in ex} == set(c["exact"]) and all(v == thr for _, v, thr in ex), (c["name"], ex)
            # and the declaration is what decides the case: under the general rule alone a margin on its threshold is undecided
            assert not am.decided(a, b)
        else:
            assert dec[-1] == am.decided(a, b)
    assert len({c["name"] for c in am.all_cases() + am.mixed_batch()}) == len(am.all_cases()) + 4
    assert sum(dec) >= 0.8 * len(cases), dec


def test_every_exit_and_level_shape_is_reached():
    ends, flags, shapes = set(), set(), set()
    for c in am.all_cases():
        m = am.case_runs(c)[0]
        lv = am.case_store(c)[2]
        ends |= {int(e) for e in m["ends"][:lv]}
        flags.add(int(m["flags"]))
        it = list(m["iters"][:lv])
        for l in range(lv - 1):
            if it[l + 1] == -1 and any(i > 0 for i in it[:l + 1]):
                shapes.add("skipped above run")
            if it[l] == -1 and it[l + 1] > 0:
                shapes.add("run above skipped")
        if m["iters"][2] > 0:
            shapes.add("iters[2]")
        if m["iters"][3] > 0:
            shapes.add("iters[3]")
        # flags is the end of the finest level that ran
        ran = [l for l in range(lv) if it[l] > 0]
        assert m["flags"] == (m["ends"][ran[0]] if ran else 0) and m["levels_run"] == len(ran)
        assert all((m["ends"][l] == -1) == (m["iters"][l] == -1) and (m["ends"][l] == 0) == (m["iters"][l] == 0) for l in range(8))
    print("ends of a level:", sorted(am.END_NAMES[e] for e in ends), "; flags:", sorted(am.END_NAMES[f] for f in flags), "; shapes:", sorted(shapes))
    five = {am.END_EPS, am.END_MAX_ITERS, am.END_CHI, am.END_PIVOT, am.END_POINTS}
    assert five <= ends and five <= flags
    assert shapes == {"skipped above run", "run above skipped", "iters[2]", "iters[3]"}


def test_the_named_edge_cases_are_what_they_are_meant_to_be():
    for t in range(4):
        for n in (40, 200):
            assert _edge("l4_t%d_n%d" % (t, n))[1]["levels_run"] == 4
    for t in range(3):
        assert _edge("odd_t%d_n100" % t)[1]["levels_run"] == 4
    # levels smaller than the patch footprint: the 9 x 6 level has no interior, the 17 x 11 level one row of it
    c, m = _edge("tiny")
    assert am.level_sizes(67, 43, 4) == [(67, 43), (34, 22), (17, 11), (9, 6)]
    print("tiny: iters %s, tvec %s (the content moves one pixel: t_x = 1/16)" % (m["iters"][:4], m["tvec"]))
    assert list(m["iters"][:4]) == [5, 5, -1, -1] and abs(m["tvec"][0] - 0.0625) <= 1e-5 and np.abs(m["tvec"][1:]).max() <= 1e-5
    c, m = _edge("tiny_min_points1")
    assert m["iters"][2] > 0 and m["iters"][3] == -1 and abs(m["tvec"][0] - 0.0625) <= 1e-5
    # the interior's comparisons on the line
    for l in range(4):
        c, m = _edge("boundary_l%d" % l)
        print("%s: used %d of 64, the six on the edges %s" % (c["name"], m["n_used"], m["used"][16 * l:16 * l + 6].astype(int)))
        assert tuple(m["used"][16 * l:16 * l + 6]) == am.BOUNDARY_USED and m["iters"][l] == 1 and m["flags"] == am.END_EPS and m["levels_run"] == 1
        assert not m["rvec"].any() and not m["tvec"].any()
        # a level's sixteen are all inside the interiors of the finer levels but for its own three outside ones
        assert m["used"][16 * l + 6:16 * l + 16].all() and m["n_used"] == int(m["used"].sum())
    # identical frames: one linearisation per level; with eps = 0 ten of them, each the tie chi == chi_prev == 0, which continues
    c, m = _edge("identical")
    assert list(m["iters"][:4]) == [1, 1, 1, 1] and m["flags"] == am.END_EPS and m["chi2"] == 0 and not m["rvec"].any() and not m["tvec"].any()
    c, m = _edge("identical_eps0")
    assert list(m["iters"][:4]) == [10, 10, 10, 10] and m["flags"] == am.END_MAX_ITERS and m["chi2"] == 0 and not m["rvec"].any() and not m["tvec"].any()
    # the pivots: stripes have gy = 0 (the second pivot; the first, H[0][0], is positive), a uniform frame has no gradient at all
    for name in ("stripes", "uniform"):
        c, m = _edge(name)
        assert list(m["iters"][:4]) == [1, 1, 1, 1] and list(m["ends"][:4]) == [am.END_PIVOT] * 4 and m["levels_run"] == 4 and m["status"] == 0
        assert m["n_used"] == 32 and m["used"].all() and not m["rvec"].any() and not m["tvec"].any()
        P = am.pyramid(c["frames"][0], 4)
        ref = am.reference(am.padded(P[0]), c["K"], 0, c["X"].astype(np.float64), pad=am.PAD)
        lin = am.linearise(ref, am.padded(P[0]), c["K"], 0, np.eye(3), np.zeros(3), 10.0, pad=am.PAD)
        assert (lin["H"][0, 0] > 0) == (name == "stripes") and lin["H"][1, 1] == 0 and not ref["gy"].any()
    # points lost while a level iterates; POINTS goes before CHI; a skipped top level above a level that runs
    c, m = _edge("leaving_points")
    assert list(m["iters"][:2]) == [10, 3] and m["ends"][1] == am.END_POINTS and m["levels_run"] == 2
    c, m = _edge("leaving_points_min_level1")
    assert list(m["iters"][:2]) == [0, 3] and m["flags"] == am.END_POINTS and m["n_used"] == 113
    c, m = _edge("leaving_top_skipped")
    assert list(m["iters"][:2]) == [10, -1] and m["levels_run"] == 1
    c, m = _edge("leaving_n200_points")
    assert list(m["iters"][:2]) == [10, 2] and m["ends"][1] == am.END_POINTS
    c, m = _edge("l4_points_top")
    assert m["ends"][3] == am.END_POINTS and m["iters"][3] == 2 and m["levels_run"] == 4
    c, m = _edge("run_above_skipped")
    assert list(m["iters"][:2]) == [-1, 1] and m["flags"] == am.END_MAX_ITERS and m["levels_run"] == 1 and m["n_used"] == 32
    c, m = _edge("points_before_chi")
    (lvl, chi, chi_prev), = m["points_exits"]
    print("points_before_chi: level %d ends by POINTS on %d points with chi %.1f after %.1f" % (lvl, 8, chi, chi_prev))
    assert lvl == 1 and chi > chi_prev and m["flags"] == am.END_POINTS and list(m["iters"][:2]) == [0, 2] and not m["rvec"].any() and not m["tvec"].any()
    c, m = _edge("chi_with_points_left")
    assert m["flags"] == am.END_CHI and list(m["iters"][:2]) == [0, 2] and not m["points_exits"] and not m["tvec"].any()
    for l in range(4):
        c, m = _edge("one_lin_l%d" % l)
        assert m["iters"][l] == 1 and m["levels_run"] == 1 and m["flags"] == am.END_MAX_ITERS and m["n_used"] >= 10
    # the count edges
    assert _edge("count_n256")[1]["n_used"] == 256 and _edge("count_n241")[1]["n_used"] == 241
    c, m = _edge("count_n241_tail11")
    assert m["n_used"] == 11 and m["used"][240] and not m["used"][:230].any()
    for name in ("count_n241_one_finite", "count_n256_one_finite", "count_n1", "count_n0"):
        c, m = _edge(name)
        assert m["status"] == am.VO_E_NUMERIC and m["levels_run"] == 0 and m["flags"] == 0 and list(m["iters"][:4]) == [-1] * 4 and not m["used"].any()
    # the mixed batch: four sequences that leave the loop at different points under one set of parameters
    mb = [am.case_runs(c)[0] for c in am.mixed_batch()]
    assert len({len(c["X"]) for c in am.mixed_batch()}) == 1 and all(c["params"] == dict(min_points=20) for c in am.mixed_batch())
    assert mb[0]["levels_run"] == 4 and mb[1]["flags"] == am.END_PIVOT and mb[2]["status"] == am.VO_E_NUMERIC and mb[3]["ends"][3] == am.END_POINTS


def test_the_padding_the_unused_points_sample_does_not_matter():
    """a point that is not used samples at (8, 8): outside a 9 x 6 level.  Whatever the border holds, the run is the same"""
    for name in ("tiny", "tiny_min_points1", "l4_t0_n40", "count_n241_tail11"):
        c, m = _edge(name)
        prev, cur = am.case_frames(c)
        lv = am.case_store(c)[2]
        P, C = am.pyramid(prev, lv), am.pyramid(cur, lv)
        for fill in (0, 255):
            for f32 in (False, True):
                want = am.case_runs(c)[1 if f32 else 0]
                got = am.run(P, C, c["K"], c["X"], c["rvec0"], c["tvec0"], f32=f32, fill=fill, **c["params"])
                assert got["rvec"].tobytes() == want["rvec"].tobytes() and got["tvec"].tobytes() == want["tvec"].tobytes()
                assert np.array_equal(got["iters"], want["iters"]) and np.array_equal(got["ends"], want["ends"]) and got["chi2"] == want["chi2"]
                assert np.array_equal(got["used"], want["used"]) and got["margins"] == want["margins"]
    # (8, 8) and its stencil do lie in the border of the tiny store's upper levels, where the bare level cannot be indexed
    c, m = _edge("tiny")
    top = am.pyramid(c["frames"][0], 4)[3]
    assert top.shape == (6, 9) and m["iters"][3] == -1
    with pytest.raises(IndexError):
        am.reference(top, c["K"], 3, c["X"].astype(np.float64))


def test_rodrigues_log_round_trip_at_the_log_exp_angles():
    """the yardstick of the log_exp cases of the GPU test: the model's own log_so3(rodrigues(r0)) - r0.  Printed; the GPU test's bound is
    8 x max(this, 2^-52 x angle).  3.0 rad and beyond are not asked for: the formula loses digits towards pi, which the header excludes"""
    for a in am.LOG_EXP_ANGLES:
        c, m = _edge("log_exp_%g" % a)
        r0 = am.log_exp_r0(a)
        err = np.abs(am.log_so3(am.rodrigues(r0)) - r0).max()
        print("angle %.1f rad: |log_so3(rodrigues(r0)) - r0| = %.3g (2^-52 x angle = %.3g); n_used %d of %d, ends %s"
              % (a, err, 2.0 ** -52 * a, m["n_used"], len(c["X"]), _ends(m, 1)))
        assert a < 3.0 and np.array_equal(c["rvec0"], r0) and abs(np.linalg.norm(r0) - a) <= 1e-15
        assert m["n_used"] == len(c["X"]) == 32 and m["ends"][0] == am.END_PIVOT and m["iters"][0] == 1 and m["levels_run"] == 1
        # the pose that comes back is T0: rvec is the round trip itself
        assert np.array_equal(m["R"], am.rodrigues(r0)) and np.array_equal(m["rvec"], am.log_so3(am.rodrigues(r0))) and not m["tvec"].any()
        assert err <= 64 * 2.0 ** -52 * a                       # (a sanity bound on the yardstick itself, not a tolerance of the kernel)
