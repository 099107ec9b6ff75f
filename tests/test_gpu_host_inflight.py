"""GPU: host-frame steps with every step the library admits in flight, against the same steps fed from the resident sequence store.

vo_pipe_step_host admits VO_PIPE_INFLIGHT closed-loop steps in flight and vo_frame_step_host two.  The gather kernel of a step reads the
device-visible addresses of that step's images from a page-locked pointer table WHILE it runs, so a table row that a later step rewrites
before the earlier gather has finished sends the earlier step's later sequences to the later step's images: no fault, silently wrong
tracks.  The reference of every comparison is the same loop on the same images from vo_seq_upload, with the same enqueue / fetch
pattern; records and tables must be bit-identical (include/vo_mi355x.h promises it), ints compared with ==, arrays with np.array_equal.

Every image is distinct: no two sequences of a step and no two steps of a sequence share one, so a step that gathered another step's
image (or another sequence's) changes that sequence's records.  Every host array a step was given stays referenced and untouched until
that step has been fetched; the loader ring refills a buffer only after the fetch of the step that used it."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VO_E_STATE = -4


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def _own(img, d, b, t):
    """sequence b's image of frame t: img + d saturating at 255 (uint8, a sequence of its own over the same geometry), and (b, t) written into
    the last three pixels of the bottom row, far from any tracked window -- a swaying camera passes every pose twice, so two frames of one
    scene can be identical"""
    out = np.minimum(img, 255 - d) + np.uint8(d) if d else img.copy()
    out[-1, -3:] = (b & 255, b >> 8, t)
    return out


@pytest.fixture(scope="module")
def world():
    """The bench's closed-loop scenes (bench.run_pipeline: pipe_scenes(2, 40, 4321)), rendered once.  Sequence b = (scene, phase offset) pair
    b % P, brightness offset b // P (P = number of pairs whose bootstrap pair (t, t + PIPE_T1) has a usable baseline), its own stamp (_own):
    256 sequences whose images are pairwise distinct within a step and within a sequence.  A sequence shares its ground-truth bootstrap state with the pairs'
    unshifted sequence (an offset moves no corner; both runs of a comparison start from the same state either way)."""
    bench = _bench()
    from vo_mi355x import VoContext, synthetic as syn
    W, H, T1 = bench.W_IMG, bench.H_IMG, bench.PIPE_T1
    scenes = bench.pipe_scenes(2, 40, 4321)
    nf = len(scenes[0]["frames"])
    goods = [list(dict.fromkeys(bench.pipe_phase_offsets(sc, nf))) for sc in scenes]
    pairs = [(k, goods[k][i]) for i in range(max(map(len, goods))) for k in range(len(scenes)) if i < len(goods[k])]
    B, n_use = 256, T1 + 1 + 9                   # the bootstrap frames, then up to 9 steps
    assert B <= 8 * len(pairs)
    boot = VoContext(W, H, max_pts=4096)
    states = {}
    try:
        for k, off in pairs:
            sc = scenes[k]
            roll = dict(frames=np.roll(sc["frames"], -off, axis=0), poses=np.roll(sc["poses"], -off, axis=0), K=sc["K"], f=sc["f"],
                        surface=lambda t, xy, sc=sc, off=off: sc["surface"]((t + off) % nf, xy))
            states[(k, off)] = syn.gt_bootstrap(boot, roll, 0, T1)[0]
    finally:
        boot.close()
    seqs = np.empty((B, n_use, H, W), np.uint8)
    seq_states, Ks = [], []
    for b in range(B):
        k, off = pairs[b % len(pairs)]
        d = b // len(pairs)
        fr = scenes[k]["frames"]
        for t in range(n_use):
            seqs[b, t] = _own(fr[(off + t) % nf], d, b, t)
        seq_states.append(states[(k, off)])
        Ks.append(scenes[k]["K"])
    return dict(bench=bench, W=W, H=H, T1=T1, seqs=seqs, states=seq_states, K=np.stack(Ks), n_use=n_use, refs={})


def _distinct(images):
    """no two arrays hold the same bytes"""
    import hashlib
    digests = [hashlib.blake2b(np.ascontiguousarray(a).data, digest_size=16).digest() for a in images]
    return len(set(digests)) == len(digests)


def _pipe(world, B, gather_workgroups=0):
    """a closed loop in the bench's w10 configuration (bench.PipeGroup: 2 048 slots, window 10, no resurrection, LM cap 10 with a fixed
    budget, default side stream) over the first B sequences of `world`"""
    from vo_mi355x import VoContext
    from vo_mi355x.resident import ResidentPipeline
    c = VoContext(world["W"], world["H"], max_pts=2048, batch=B)
    if gather_workgroups:
        c.set_tuning(gather_workgroups=gather_workgroups)
    rp = ResidentPipeline(c, world["K"][:B], ba_window=10, ba_max_iters=10, ba_budget=10, pnp_blind_batches=2, resurrect=False)
    rp.seed(world["states"][:B], None, None, t_step=1)
    return c, rp


def _drive(rp, enqueue, n_steps, after_fetch=None, when_full=None):
    """INFLIGHT steps back to back from the first, then one fetch + one enqueue until done, then drain; after_fetch(s) runs once step s is
    fetched, when_full() whenever INFLIGHT steps are in flight -> the records, oldest first"""
    from vo_mi355x.resident import INFLIGHT
    recs = []

    def fetch():
        recs.append(rp.fetch())
        if after_fetch is not None:
            after_fetch(len(recs) - 1)
    for s in range(n_steps):
        if s >= INFLIGHT:
            if when_full is not None:
                when_full()
            fetch()
        enqueue(s)
    while len(recs) < n_steps:
        fetch()
    return recs


def _resident_run(world, B, n_steps, gather_workgroups=0):
    """the reference: the same loop with every frame from the resident sequence store (cached per shape)"""
    key = (B, n_steps, gather_workgroups)
    if key not in world["refs"]:
        T1 = world["T1"]
        c, rp = _pipe(world, B, gather_workgroups)
        try:
            c.upload_sequence(world["seqs"][:B, :T1 + 1 + n_steps])
            c.push_frame_resident(T1)
            recs = _drive(rp, lambda s: rp.step(T1 + 1 + s), n_steps)
            world["refs"][key] = (recs, rp.read_tables())
        finally:
            c.close()
    return world["refs"][key]


def _same_value(x, y):
    if isinstance(x, dict):
        return x.keys() == y.keys() and all(_same_value(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)):
        return len(x) == len(y) and all(_same_value(a, b) for a, b in zip(x, y))
    if isinstance(x, np.ndarray):
        return x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f")
    return x == y or (x != x and y != y)


def _assert_same(got, ref, what):
    """records step by step, sequence by sequence, every field; then every table.  On a difference: per sequence the first step whose
    record differs (the step that saw an image not its own changes there first) and the fields that differ"""
    got_recs, got_T = got
    ref_recs, ref_T = ref
    assert len(got_recs) == len(ref_recs)
    first_bad = {}
    for s, (gs, rs) in enumerate(zip(got_recs, ref_recs)):
        gs, rs = (gs, rs) if isinstance(gs, list) else ([gs], [rs])
        for b, (g, r) in enumerate(zip(gs, rs)):
            assert g.keys() == r.keys()
            bad = [k for k in r if not _same_value(g[k], r[k])]
            if bad and b not in first_bad:
                first_bad[b] = (s, bad)
    assert not first_bad, "%s: %d sequences differ; (sequence: first step, fields) %s" % (
        what, len(first_bad), sorted(first_bad.items())[:16])
    for name in ref_T:
        assert _same_value(got_T[name], ref_T[name]), (what, name)


def _steps_images(world, B, n_steps):
    """[step][sequence] -> the image of that step (views into the sequence stack), checked pairwise distinct within a step and a sequence"""
    T1 = world["T1"]
    imgs = [[world["seqs"][b, T1 + 1 + s] for b in range(B)] for s in range(n_steps)]
    assert all(_distinct(step) for step in imgs), "two sequences of a step share an image"
    assert all(_distinct([imgs[s][b] for s in range(n_steps)]) for b in range(B)), "two steps of a sequence share an image"
    return imgs


def _host_run(world, B, n_steps, source, gather_workgroups=0):
    """the loop with every step's images handed over by the host from `source`; every array stays referenced until the run is over"""
    from vo_mi355x import VoContext
    from vo_mi355x.resident import INFLIGHT
    T1, H, W = world["T1"], world["H"], world["W"]
    imgs = _steps_images(world, B, n_steps)
    after_fetch = None
    if source == "pinned":            # a distinct page-locked array for every (sequence, step)
        store = VoContext.host_alloc((n_steps, B, H, W))
        for s in range(n_steps):
            store[s] = np.stack(imgs[s])
        give = [[store[s, b] for b in range(B)] for s in range(n_steps)]
    elif source == "strided":         # page-locked rows of 1 280 bytes holding 1 241: the gather's per-row branch, rows with a 9-byte tail
        store = VoContext.host_alloc((n_steps, B, H, 1280))
        for s in range(n_steps):
            store[s, :, :, :W] = np.stack(imgs[s])
        give = [[store[s, b, :, :W] for b in range(B)] for s in range(n_steps)]
    elif source == "pageable":        # the sequence stack itself: pageable, one array per (sequence, step)
        store = None
        give = imgs
    elif source == "ring":            # a loader's ring of INFLIGHT page-locked buffers per sequence: buffer s % INFLIGHT is refilled with the
        store = VoContext.host_alloc((INFLIGHT, B, H, W))     # image of step s + INFLIGHT only after step s has been fetched
        for s in range(min(INFLIGHT, n_steps)):
            store[s] = np.stack(imgs[s])
        give = [[store[s % INFLIGHT, b] for b in range(B)] for s in range(n_steps)]

        def after_fetch(s):
            if s + INFLIGHT < n_steps:
                store[s % INFLIGHT] = np.stack(imgs[s + INFLIGHT])
    else:
        raise ValueError(source)
    c, rp = _pipe(world, B, gather_workgroups)
    try:
        sets = [c.host_frames(g) for g in give]
        if source == "ring":
            assert all(sets[s][0][b] == sets[s % INFLIGHT][0][b] for s in range(n_steps) for b in range(B))     # the same buffers again
        c.push_frame(world["seqs"][:B, T1])
        recs = _drive(rp, lambda s: rp.step_host(sets[s]), n_steps, after_fetch)
        out = (recs, rp.read_tables())
    finally:
        c.close()
    del store
    return out


def test_bench_shape_all_pipe_steps_in_flight_from_the_first(world):
    """bench.py --workload pipeline --pipe-host-frames at its w10 configuration: 256 sequences at 1241 x 376 in one context, VO_PIPE_INFLIGHT
    host steps enqueued back to back from the first (each gather moves 119 MB over PCIe, ~2 ms), then one fetch + one enqueue; 8 steps with a
    distinct page-locked array per (sequence, step) (~0.95 GB) = the resident loop"""
    B, n = 256, 8
    ref = _resident_run(world, B, n)
    _assert_same(_host_run(world, B, n, "pinned"), ref, "256 x 1241x376, pinned")


@pytest.mark.parametrize("source", ["pinned", "ring", "strided", "pageable"])
def test_slow_gather_all_pipe_steps_in_flight(world, source):
    """16 sequences at 1241 x 376 with ONE gather workgroup (vo_tuning.gather_workgroups = 1): each step's gather takes 2.35 ms (kernel trace
    on an MI355X: 7.5 MB at ~3.2 GB/s), so the later steps are enqueued while the first one is still reading its pointer table -- the window
    held open on purpose"""
    B, n = 16, 8
    ref = _resident_run(world, B, n, gather_workgroups=1)
    _assert_same(_host_run(world, B, n, source, gather_workgroups=1), ref, "16 x 1241x376, one gather workgroup, " + source)


def test_refused_host_steps_leave_no_trace(world):
    """Every refusal of vo_pipe_step_host that a caller can reach -- no frame in the store yet, VO_PIPE_INFLIGHT steps in flight, a frame step in
    flight on the gated stream layout -- raises VO_E_STATE, and the steps after it (one gather workgroup: every gather still running when the next
    steps come) equal those of a context that never saw the refused calls, record for record and table for table"""
    from vo_mi355x import VoContext, VoError
    B, n_loop, n_after = 16, 6, 2
    T1, H, W = world["T1"], world["H"], world["W"]
    n_img = n_loop + 1 + n_after                 # the loop's steps, one frame step, the steps after it
    imgs = _steps_images(world, B, n_img)
    store = VoContext.host_alloc((n_img, B, H, W))
    for s in range(n_img):
        store[s] = np.stack(imgs[s])

    def refuse(c, rp, s):
        inflight = rp._inflight
        with pytest.raises(VoError) as e:
            rp.step_host(c.host_frames([store[s, b] for b in range(B)]))
        assert e.value.code == VO_E_STATE, str(e.value)
        assert rp._inflight == inflight

    def run(refusing):
        c, rp = _pipe(world, B, gather_workgroups=1)
        try:
            sets = [c.host_frames([store[s, b] for b in range(B)]) for s in range(n_img)]
            if refusing:
                refuse(c, rp, 0)                                     # nothing pushed yet: tracking needs two frames in the store
            c.push_frame(world["seqs"][:B, T1])
            full = (lambda: refuse(c, rp, n_loop)) if refusing else None     # INFLIGHT steps already in flight
            recs = _drive(rp, lambda s: rp.step_host(sets[s]), n_loop, when_full=full)
            tables = rp.read_tables()
            # a frame step on the gated layout (a batch's pipelined stream layout), in flight while the loop is asked for a step
            c.set_side_stream("pipeline")
            assert c.step_layout()["reserved_cus"] > 0
            c.frame_step_host(sets[n_loop], c.max_pts, do_dlt=False, do_ba=False, do_st=False)
            if refusing:
                refuse(c, rp, n_loop + 1)
            fr = c.frame_fetch()
            recs2 = _drive(rp, lambda s: rp.step_host(sets[n_loop + 1 + s]), n_after)
            return (recs, tables), fr, (recs2, rp.read_tables())
        finally:
            c.close()

    ref = run(False)
    got = run(True)
    _assert_same(got[0], ref[0], "after refusals: no frame, INFLIGHT in flight")
    for k in ref[1]:
        assert _same_value(got[1][k], ref[1][k]), ("frame step", k)
    _assert_same(got[2], ref[2], "after a refusal on the gated layout")


@pytest.fixture(scope="module")
def headline_host_run():
    """bench.Group at the headline's shape and layout (256 sequences, vo_set_side_stream "pipeline": the gather runs 2 parts per image on 512
    workgroups beside the tracker), three frame steps with two in flight: once from the resident store, once with 256 distinct page-locked images
    per step.  Sequence b's images: bench sequence b % 8 with a brightness offset b // 8 and its own stamp (bench.Group serves 256 sequences from 8, so a mix-up of
    sequences b and b + 8 would not show).  The context is closed before the tests look."""
    bench = _bench()
    from vo_mi355x import synthetic as syn
    W, H, N, B, n_steps = bench.W_IMG, bench.H_IMG, bench.N_PTS, 256, 3
    frame_sets = [syn.make_sequence(100, W, H, seed=1234 + k, periodic=True, n_render=n_steps + 2)[0] for k in range(8)]
    seqs = np.stack([np.stack([_own(f, b // 8, b, t) for t, f in enumerate(frame_sets[b % 8])]) for b in range(B)])       # [B][5][H][W]
    for t in range(1, n_steps + 1):
        assert _distinct(list(seqs[:, t])), t
    g = bench.Group(0, frame_sets, seed0=0, batch=B, ba_iters=30)
    try:
        c = g.c
        c.upload_sequence(seqs)
        c.set_side_stream("pipeline")
        assert c.step_layout() == {"layout": 2, "gate_groups": 4, "reserved_cus": 32}
        pts0 = np.stack([syn.grid_points(N, W, H, seed=b) for b in range(B)])

        def run(host):
            c.points_upload(pts0)
            c.push_frame_resident(0)
            g.t, g.host = 1, host
            out = []
            for _ in range(n_steps):
                g.enqueue()
                if g.inflight == 2:
                    g.fetch(); out.append(g.last)
            while g.inflight:
                g.fetch(); out.append(g.last)
            return out
        ref = run(None)
        store = c.host_alloc((n_steps + 2, B, H, W))
        store[:] = seqs.transpose(1, 0, 2, 3)
        host = [c.host_frames([store[f, b] for b in range(B)]) for f in range(n_steps + 2)]
        got = run(host)
        # the last two steps were in flight together: their level-0 images, every sequence
        lvl0 = [[c.pyramid_read(which, 0, seq=b)[0] for b in range(B)] for which in (0, 1)]
        g.host = None
    finally:
        g.c.close()
    return dict(ref=ref, got=got, lvl0=lvl0, seqs=seqs, n_steps=n_steps, B=B)


def test_frame_step_host_headline_level0_is_each_sequences_own_image(headline_host_run):
    R = headline_host_run
    seqs, n, B = R["seqs"], R["n_steps"], R["B"]
    bad = [(t, b) for which, t in ((0, n - 1), (1, n)) for b in range(B) if not np.array_equal(R["lvl0"][which][b], seqs[b, t])]
    assert not bad, "level 0 is not the sequence's own image at (frame, sequence) %s" % bad[:16]


def test_frame_step_host_headline_equals_resident(headline_host_run):
    R = headline_host_run
    for s, (g, r) in enumerate(zip(R["got"], R["ref"])):
        assert g.keys() == r.keys()
        for k in r:
            assert _same_value(g[k], r[k]), (s, k)
