"""Cost of the oriented BRIEF descriptor (vo_set_brief; k_brief_describe) on the detection launch group, and of the Hamming matcher against
the float L2 matcher, in one process.

1. vo_tracks_detect on `seqs` sequences of 1241x376 with the setting off and on, alternating over ROUNDS rounds, for
     steady  1000 live tracks on a grid with exclusion discs wide enough (radius 12 / 14) to cover most of the image: few new corners, as in
             the middle of a sequence whose tracks already sit on the corners (discs of radius 7 on a grid leave this scene 1000 new ones)
     first   one live track, radius 7: the detection fills max_corners = 1000 corners (a first frame)
   The corner count of sequence 0 is printed with every line: it says which of the two a line measured.
   max_new = 0, so no track is spawned and every launch sees the same table; the kernel still describes every detected corner.
   Time: host clock around LAUNCHES enqueues that end in a device synchronise (what a launch group costs in a stream), after WARM launches.
2. vo_match_hamming_knn2 at 1000 x 1000 x 32 bytes against vo_match_knn2 at 1000 x 1000 x 128 float32, batch 1, both synchronous calls
   with their uploads and read-backs (that is the call a user makes), alternating.
The per-kernel times come from a kernel trace of the same loops, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ks -- python3 tools/brief_timing.py 64 trace
    python3 tools/brief_timing.py DIR            # prints k_brief_describe, k_st_*, k_match_* from DIR/**/*kernel_stats.csv
usage: tools/brief_timing.py [seqs] [trace]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-odom-pipeline_amd"))
import numpy as np

ROUNDS, WARM, LAUNCHES, MATCHES = 3, 10, 300, 30

if len(sys.argv) > 1 and os.path.isdir(sys.argv[1]):
    import csv, glob
    f = sorted(glob.glob(os.path.join(sys.argv[1], "**", "*kernel_stats.csv"), recursive=True))[-1]
    for r in csv.DictReader(open(f)):
        name = r["Name"].split("(")[0].replace("void ", "")
        if name.startswith(("k_st_", "k_brief_", "k_match_", "k_trk_spawn")):
            print("%-28s calls %5s avg %8.1f us  total %10.1f us" % (name[:28], r["Calls"], float(r["AverageNs"]) / 1e3, float(r["TotalDurationNs"]) / 1e3))
    sys.exit(0)

from vo_mi355x import VoContext, synthetic as syn
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
W, H, N = 1241, 376, 1000
one = syn.make_sequence(1, w=W, h=H, seed=3, margin=64)[0]
frames = np.ascontiguousarray(np.broadcast_to(one, (B, 1, H, W)))
for case, n_live, radius in (("steady r12", N, 12), ("steady r14", N, 14), ("first", 1, 7)):
    pts = syn.grid_points(n_live, W, H, seed=1)
    with VoContext(W, H, max_pts=2048, batch=B) as c:
        c.upload_sequence(frames)
        c.push_frame_resident(0)
        c.tracks_seed(np.ascontiguousarray(np.broadcast_to(pts, (B, n_live, 2))) if B > 1 else pts, t=0)
        prm = c.st_params()
        for rnd in range(ROUNDS):
            for on in (False, True):
                c.set_brief(True if on else None)
                for k in range(WARM):
                    c.tracks_detect(0, radius, prm, max_new=0)
                c.sync()
                t0 = time.perf_counter()
                for k in range(LAUNCHES):
                    c.tracks_detect(0, radius, prm, max_new=0)
                c.sync()
                dt = time.perf_counter() - t0
                n = len(c.shi_tomasi_fetch()[0]) if B > 1 else len(c.shi_tomasi_fetch())
                print("%-10s B=%d round %d brief %-3s: detection launch group %8.1f us (%d launches, window %.2f s), %d corners in sequence 0" %
                      (case, B, rnd, "on" if on else "off", 1e6 * dt / LAUNCHES, LAUNCHES, dt, n), flush=True)

rs = np.random.RandomState(0)
n1 = n2 = 1000
b1, b2 = rs.randint(0, 256, (n1, 32)).astype(np.uint8), rs.randint(0, 256, (n2, 32)).astype(np.uint8)
f1, f2 = rs.rand(n1, 128).astype(np.float32), rs.rand(n2, 128).astype(np.float32)
with VoContext(320, 240, max_pts=64) as c:
    for rnd in range(ROUNDS):
        for name, fn in (("hamming 1000 x 1000 x 32 B", lambda: c.match_hamming_knn2(b1, b2)), ("L2 1000 x 1000 x 128 f32", lambda: c.match_knn2(f1, f2))):
            for k in range(3):
                fn()
            t0 = time.perf_counter()
            for k in range(MATCHES):
                fn()
            dt = time.perf_counter() - t0
            print("match round %d %-28s: %8.1f us per synchronous call (%d calls)" % (rnd, name, 1e6 * dt / MATCHES, MATCHES), flush=True)
