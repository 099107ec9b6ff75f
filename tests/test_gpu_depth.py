"""GPU: the depth filter (vo_depth_seed_init, vo_depth_update, csrc/vo_depth.hip) through the C ABI against tests/depth_model.py, on the seeds
tests/test_depth_model.py shows the model to decide on its own.  Frames 208 x 120 and 131 x 77.  run_case() also serves
tests/test_gpu_depth_edges.py.

A case is a chain: the seeds are made once and updated against one frame after the other, the kernel's state carried by the kernel and the
model's by the model, so a drift would accumulate.  Discrete outcomes (result codes, flags, the counts, the best candidate where the call
reports it) are equal.  Tolerance of the continuous outputs (match_uv, z, mu, sigma2, a, b), per case, frame and output: the largest
deviation of the kernel from the float64 model over the decided seeds, against FACTOR = 4 x the largest deviation of the model's own
float32 switch (a chain of its own) -- the rule and the factor of tests/test_gpu_align.py; match_uv comes back as float32, so it is allowed
one rounding of that format (2^-24 relative) on top.  Where the switch moves an output by nothing at all the bound is 1e-12 relative, and
the test prints which those are.  Every ratio is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

import depth_model as dm

pytestmark = pytest.mark.gpu
FACTOR = 4.0
INVALID, STATE, CAPACITY = -1, -4, -5


def _p(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def raw_seed_init(ctx, uv, depth_mean, depth_min, ref_id=0, n=None):
    """vo_depth_seed_init itself -> (return code, seeds [B, n], patches [B, n, 100], ok [B, n])"""
    from vo_mi355x import _lib
    L, B = _lib.load(), ctx.batch
    uv = np.ascontiguousarray(uv, np.float32).reshape(B, -1, 2)
    n = uv.shape[1] if n is None else n
    rows = max(uv.shape[1], 1)
    dmean = np.ascontiguousarray(np.broadcast_to(np.asarray(depth_mean, np.float64).reshape(-1), (B,)))
    dmin = np.ascontiguousarray(np.broadcast_to(np.asarray(depth_min, np.float64).reshape(-1), (B,)))
    seeds, patches, ok = np.zeros((B, rows), dm.SEED), np.full((B, rows, 100), 255, np.uint8), np.full((B, rows), 255, np.uint8)
    rc = L.vo_depth_seed_init(ctx._h, _p(uv, C.c_float), n, _p(dmean, C.c_double), _p(dmin, C.c_double), ref_id, _p(seeds, _lib.DepthSeed),
                              _p(patches, C.c_uint8), _p(ok, C.c_uint8))
    return rc, seeds[:, :uv.shape[1]], patches[:, :uv.shape[1]], ok[:, :uv.shape[1]]


def raw_update(ctx, K, poses, seeds, patches, prm=None, n=None, **params):
    """vo_depth_update itself; seeds [B, n] (or [n]) is updated in place -> (return code, result [B, n], match_uv [B, n, 2], z [B, n],
    stats [B, 9] (the seven counts, converged, diverged))"""
    from vo_mi355x import _lib
    L, B = _lib.load(), ctx.batch
    K = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (B, 3, 3)))
    poses = np.ascontiguousarray(poses, np.float64).reshape(B, -1, 6)
    s = seeds.reshape(B, -1)
    assert s.flags["C_CONTIGUOUS"] and np.shares_memory(s, seeds)
    rows = s.shape[1]
    n = rows if n is None else n
    patches = np.ascontiguousarray(patches, np.uint8).reshape(B, rows, 100)
    if prm is None:
        prm = ctx.depth_params(**params)
    res, match, z = np.full((B, max(rows, 1)), 255, np.uint8), np.full((B, max(rows, 1), 2), -1.0, np.float32), np.full((B, max(rows, 1)), -1.0)
    st = (_lib.DepthStats * B)()
    rc = L.vo_depth_update(ctx._h, _p(K, C.c_double), _p(poses, C.c_double), poses.shape[1], _p(s, _lib.DepthSeed), _p(patches, C.c_uint8), n,
                           C.byref(prm), _p(res, C.c_uint8), _p(match, C.c_float), _p(z, C.c_double), st)
    stats = np.array([list(x.counts) + [x.converged, x.diverged] for x in st], np.int32)
    return rc, res[:, :rows], match[:, :rows], z[:, :rows], stats


class Stores:
    """one context per (frame size, batch), opened when first asked for"""

    def __init__(self):
        self.open = {}

    def get(self, size, batch=1):
        from vo_mi355x import VoContext
        if (size, batch) not in self.open:
            self.open[(size, batch)] = VoContext(size[0], size[1], max_pts=320, batch=batch)
        return self.open[(size, batch)]

    def close(self):
        for c in self.open.values():
            c.close()
        self.open = {}


@pytest.fixture(scope="module")
def stores():
    s = Stores()
    yield s
    s.close()


RATIOS = {}


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def compare_step(name, k, got, st, rows, record=True):
    """one update of the kernel (got: seeds, result, match_uv, z, stats) against the model's step st on the seeds `rows` (a bool mask)"""
    m64, m32 = st["m64"], st["m32"]
    seeds, res, match, z, stats = got
    assert np.array_equal(res[rows], m64["result"][rows]), (name, k, np.nonzero(rows & (res != m64["result"]))[0][:8])
    assert np.array_equal(seeds["flags"][rows], m64["seeds"]["flags"][rows])
    assert np.array_equal(np.bincount(res, minlength=7)[:7], stats[:7]) and int(((seeds["flags"] & 1) != 0).sum()) == stats[7] and \
        int(((seeds["flags"] & 2) != 0).sum()) == stats[8]
    if rows.all():
        assert np.array_equal(stats, m64["stats"]), (stats, m64["stats"])
    for key in ("z_range", "u", "v", "ref_id"):                      # what no update touches
        assert seeds[key].tobytes() == m64["seeds"][key].tobytes()
    # the best candidate itself, where the call reports it: an outlier without a match comes back at its pixel (plus the seed's own offset)
    nm = rows & (m64["result"] == dm.OUTLIER_NOMATCH)
    off = np.stack([seeds["u"], seeds["v"]], 1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        off = off - np.floor(off + 0.5)
    assert np.array_equal(np.round(match[nm].astype(np.float64) - off[nm]).astype(np.int64), m64["best_px"][nm])
    kern = dict(match_uv=match.astype(np.float64), z=z, mu=seeds["mu"], sigma2=seeds["sigma2"], a=seeds["a"], b=seeds["b"])
    c64, c32 = dm.continuous(m64), dm.continuous(m32)
    worst = 0.0
    for key in dm.CONTINUOUS:
        a, b64, b32 = kern[key][rows], c64[key][rows], c32[key][rows]
        assert same_nan(a, b64), (name, k, key)
        fin = np.isfinite(b64) & np.isfinite(b32)
        if not fin.any():
            continue
        with np.errstate(invalid="ignore"):
            dev = np.abs(a - b64)[fin].max()
            d32 = np.abs(b32 - b64)[fin].max()
        fmt = 2.0 ** -24 * np.abs(b64[fin]).max() if key == "match_uv" else 0.0
        if d32 > 0:
            ratio = max(dev - fmt, 0.0) / d32
            print("%s frame %d %-8s kernel - model %.3g, float32 switch - model %.3g, ratio %.3g (bound %g)%s"
                  % (name, k, key, dev, d32, ratio, FACTOR, "" if not fmt else "; one float32 rounding %.3g taken off" % fmt))
            assert dev <= FACTOR * d32 + fmt, (name, k, key)
            worst = max(worst, ratio)
        else:
            scale = np.abs(b64[fin]).max()
            print("%s frame %d %-8s the float32 switch moves nothing: kernel - model %.3g against 1e-12 x %.3g" % (name, k, key, dev, scale))
            assert dev <= 1e-12 * scale + fmt, (name, k, key)
    if record:
        RATIOS[(name, k)] = worst
    return worst


def run_case(ctx, case, rows_extra=None):
    """a case of depth_model.gpu_cases() / edge_cases() on the batch-1 context ctx -> list per frame of (seeds, result, match_uv, z, stats)"""
    d = dm.case_data(case)
    steps = dm.case_runs(case)
    if "uv" in case:
        ctx.push_frame(d["ref"])
        rc, seeds, patches, ok = raw_seed_init(ctx, case["uv"], case["depth_mean"], case["depth_min"])
        assert rc == 0
        assert patches[0].tobytes() == d["patches"].tobytes() and seeds[0].tobytes() == d["seeds"].tobytes() and np.array_equal(ok[0], d["ok"])
        seeds, patches = seeds[0].copy(), patches[0]
    else:
        seeds, patches = d["seeds"].copy(), d["patches"]
    out = []
    for k, ((img, poses), st) in enumerate(zip(d["steps"], steps)):
        ctx.push_frame(img)
        rc, res, match, z, stats = raw_update(ctx, d["K"], poses, seeds, patches, **case["params"])
        assert rc == 0
        rows = st["decided"] if rows_extra is None else (st["decided"] | rows_extra)
        print("%s frame %d: %d seeds, %d decided by the model alone; kernel's counts %s" % (case["name"], k, len(seeds), int(st["decided"].sum()), stats[0].tolist()))
        compare_step(case["name"], k, (seeds, res[0], match[0], z[0], stats[0]), st, rows)
        out.append((seeds.copy(), res[0].copy(), match[0].copy(), z[0].copy(), stats[0].copy()))
    return out


@pytest.mark.parametrize("case", dm.gpu_cases(), ids=lambda c: c["name"])
def test_kernel_against_model(stores, case):
    got = run_case(stores.get(case["size"]), case)
    if case["name"] == "chain_n200":
        sd = got[-1][0]
        sc = dm.scene(*case["size"])
        conv = (sd["flags"] & dm.CONVERGED) != 0
        err = np.abs(sd["mu"] - dm.true_mu(sc, case["uv"])) / np.sqrt(sd["sigma2"])
        print("   after %d frames %d of %d seeds have converged; their median error is %.3f sigma" % (len(got), int(conv.sum()), len(sd), np.median(err[conv])))
        assert conv.sum() >= 50 and np.median(err[conv]) < 1.0


def test_largest_ratio_over_the_cases(stores):
    """the figure DESIGN.md records (the tests above have left their ratios; a case that did not run is run here)"""
    for case in dm.gpu_cases():
        if (case["name"], 0) not in RATIOS:
            run_case(stores.get(case["size"]), case)
    k = max(RATIOS, key=RATIOS.get)
    print("largest (kernel - model) / (float32 switch - model) over %d updates: %.3g (%s frame %d); bound %g" % (len(RATIOS), RATIOS[k], k[0], k[1], FACTOR))
    assert RATIOS[k] <= FACTOR


def test_batch_positions_and_repeated_calls_are_bit_equal(stores):
    """batch 3, sequence 1 a copy of sequence 0: bit-equal to each other and to the batch-1 call; a repeated call is bit-equal"""
    a, c = (x for x in dm.gpu_cases() if x["name"] in ("chain_n200", "n257_edges"))
    da, dc = dm.case_data(a), dm.case_data(c)
    n = 200
    K = np.stack([da["K"], da["K"], dc["K"]])
    (img_a, pose_a), (img_c, pose_c) = da["steps"][2], dc["steps"][0]
    poses = np.stack([pose_a, pose_a, pose_c])
    cb = stores.get(a["size"], batch=3)
    cb.push_frame(np.stack([da["ref"], da["ref"], dc["ref"]]))
    rc, s0, p0, ok0 = raw_seed_init(cb, np.stack([a["uv"][:n], a["uv"][:n], c["uv"][:n]]), dm.DEPTH_MEAN, dm.DEPTH_MIN)
    assert rc == 0 and s0[0].tobytes() == s0[1].tobytes() == da["seeds"][:n].tobytes() and p0[0].tobytes() == p0[1].tobytes()
    assert s0[2].tobytes() == dc["seeds"][:n].tobytes() and p0[2].tobytes() == dc["patches"][:n].tobytes()
    cb.push_frame(np.stack([img_a, img_a, img_c]))
    s1, s2 = s0.copy(), s0.copy()
    got = raw_update(cb, K, poses, s1, p0)
    again = raw_update(cb, K, poses, s2, p0)
    assert got[0] == again[0] == 0 and s1.tobytes() == s2.tobytes() and all(got[k].tobytes() == again[k].tobytes() for k in (1, 2, 3, 4))
    assert s1[0].tobytes() == s1[1].tobytes() and all(got[k][0].tobytes() == got[k][1].tobytes() for k in (1, 2, 3, 4))
    assert s1[0].tobytes() != s1[2].tobytes() and s1[0].tobytes() != s0[0].tobytes()
    c1 = stores.get(a["size"])
    for b, (d, img, pose) in enumerate(((da, img_a, pose_a), (da, img_a, pose_a), (dc, img_c, pose_c))):
        c1.push_frame(img)
        s = s0[b].copy()
        one = raw_update(c1, d["K"], pose, s, p0[b])
        assert one[0] == 0 and s.tobytes() == s1[b].tobytes() and all(one[k][0].tobytes() == got[k][b].tobytes() for k in (1, 2, 3, 4))


def test_error_codes_enqueue_nothing():
    from vo_mi355x import VoContext, _lib
    (case,) = [c for c in dm.gpu_cases() if c["name"] == "steps8_n64"]
    d = dm.case_data(case)
    K, (img, poses), uv = d["K"], d["steps"][0], case["uv"]
    L = _lib.load()
    with VoContext(dm.W, dm.H, max_pts=128) as c:
        assert raw_seed_init(c, uv, 8.0, 3.0)[0] == STATE                              # no frame pushed
        assert raw_update(c, K, poses, d["seeds"].copy(), d["patches"])[0] == STATE
        c.push_frame(d["ref"])
        rc, seeds, patches, ok = raw_seed_init(c, uv, dm.DEPTH_MEAN, dm.DEPTH_MIN)
        assert rc == 0 and seeds[0].tobytes() == d["seeds"].tobytes()
        c.push_frame(img)
        s_want = seeds[0].copy()
        want = raw_update(c, K, poses, s_want, patches[0])
        assert want[0] == 0 and want[4][0][:7].sum() == len(uv)
        big = np.zeros(129, dm.SEED)
        assert raw_update(c, K, poses, big, np.zeros((129, 100), np.uint8))[0] == CAPACITY
        assert raw_seed_init(c, np.zeros((129, 2), np.float32), 8.0, 3.0)[0] == CAPACITY
        for bad in (dict(max_steps=0), dict(max_steps=129), dict(max_iters=0), dict(max_score=-1), dict(max_score=4161601), dict(eps_align=float("nan")),
                    dict(eps_align=-1.0), dict(px_noise=float("nan")), dict(px_noise=-0.5), dict(conv_ratio=float("nan")), dict(conv_ratio=-1.0), dict(conv_ratio=0.0), dict(conv_ratio=float("inf")),
                    dict(min_inlier=float("nan")), dict(min_inlier=-0.1), dict(px_noise=float("inf"))):
            s = seeds[0].copy()
            assert raw_update(c, K, poses, s, patches[0], **bad)[0] == INVALID, bad
            assert s.tobytes() == seeds[0].tobytes()
        s = seeds[0].copy()
        assert raw_update(c, K, poses, s, patches[0], n=-1)[0] == INVALID
        assert raw_seed_init(c, uv, 8.0, 3.0, n=-1)[0] == INVALID
        for dmean, dmin in ((0.0, 3.0), (8.0, 0.0), (float("nan"), 3.0), (8.0, float("inf")), (-8.0, 3.0)):
            assert raw_seed_init(c, uv, dmean, dmin)[0] == INVALID
        Kc, pc = np.ascontiguousarray(K, np.float64), np.ascontiguousarray(poses, np.float64)
        sp, pp = _p(s, _lib.DepthSeed), _p(np.ascontiguousarray(patches[0]), C.c_uint8)
        assert L.vo_depth_update(c._h, _p(Kc, C.c_double), _p(pc, C.c_double), 0, sp, pp, len(s), None, None, None, None, None) == INVALID      # n_ref < 1
        assert L.vo_depth_update(c._h, None, _p(pc, C.c_double), 1, sp, pp, len(s), None, None, None, None, None) == INVALID
        assert L.vo_depth_update(c._h, _p(Kc, C.c_double), None, 1, sp, pp, len(s), None, None, None, None, None) == INVALID
        assert L.vo_depth_update(c._h, _p(Kc, C.c_double), _p(pc, C.c_double), 1, None, pp, len(s), None, None, None, None, None) == INVALID
        assert L.vo_depth_update(c._h, _p(Kc, C.c_double), _p(pc, C.c_double), 1, sp, None, len(s), None, None, None, None, None) == INVALID
        assert L.vo_depth_update(None, None, None, 1, None, None, 0, None, None, None, None, None) == INVALID
        assert L.vo_depth_seed_init(None, None, 0, None, None, 0, None, None, None) == INVALID
        assert L.vo_depth_default_params(None) == INVALID
        assert s.tobytes() == seeds[0].tobytes()
        # a step in flight
        sc = dm.scene(dm.W, dm.H)
        c.upload_sequence(sc["frames"][:3])
        c.push_frame_resident(0)
        p = np.array([[50.0, 40.0], [100.0, 60.0], [150.0, 80.0]], np.float32)
        c.points_upload(p)
        c.frame_step_resident(1, len(p), do_dlt=False, do_ba=False, do_st=False)
        assert raw_update(c, K, poses, s, patches[0])[0] == STATE and raw_seed_init(c, uv, 8.0, 3.0)[0] == STATE
        c.frame_fetch()
        assert s.tobytes() == seeds[0].tobytes()
        # nothing was left enqueued: the valid call gives the bits it gave before; outputs may be NULL, and NULL parameters are the defaults
        c.push_frame(img)
        got = raw_update(c, K, poses, s, patches[0])
        assert got[0] == 0 and s.tobytes() == s_want.tobytes() and all(got[k].tobytes() == want[k].tobytes() for k in (1, 2, 3, 4))
        s2 = seeds[0].copy()
        assert L.vo_depth_update(c._h, _p(Kc, C.c_double), _p(pc, C.c_double), 1, _p(s2, _lib.DepthSeed), pp, len(s2), None, None, None, None, None) == 0
        assert s2.tobytes() == s_want.tobytes()
