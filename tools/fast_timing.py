"""Cost of the detection launch group with the FAST-9/16 response (vo_st_params.fast_threshold) and with the default Shi-Tomasi response, in one
process on the same frames: 256 sequences of 1241x376, 1000 exclusion discs each, resident launches (vo_shi_tomasi_resident).

Region time from the library's own profile scope (VO_PROF_ST: every launch of the group -- mask, discs, response, NMS, selection), the two
detectors alternating over three rounds.  The per-kernel split (k_fast_score, k_st_nms, k_st_select against k_st_eig_fused, k_st_select) comes
from a kernel trace of the same loop, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ks -- python3 tools/fast_timing.py 256 scene trace
    python3 tools/fast_timing.py DIR            # prints the table from DIR/**/*kernel_stats.csv
usage: tools/fast_timing.py [seqs] [image: scene | noise | flat] [trace]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-odom-pipeline_amd"))
import numpy as np

ROUNDS, WARM, LAUNCHES = 3, 5, 30

if len(sys.argv) > 1 and os.path.isdir(sys.argv[1]):
    import csv, glob
    f = sorted(glob.glob(os.path.join(sys.argv[1], "**", "*kernel_stats.csv"), recursive=True))[-1]
    per = ROUNDS * (WARM + LAUNCHES)                  # launches of each detector in a trace run
    for r in csv.DictReader(open(f)):
        name = r["Name"].split("(")[0].replace("void ", "")
        if name.startswith(("k_st_", "k_fast_")):
            print("%-28s calls %5s avg %8.1f us  per detection launch group %8.1f us" % (name[:28], r["Calls"], float(r["AverageNs"]) / 1e3,
                                                                                      float(r["TotalDurationNs"]) / 1e3 / per))
    print("(k_st_nms runs only in the FAST group; k_st_select, k_st_discs in both: their `per group` column is over one detector's %d launches)" % per)
    sys.exit(0)

from vo_mi355x import VoContext, synthetic as syn
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
kind = sys.argv[2] if len(sys.argv) > 2 else "scene"
trace = len(sys.argv) > 3 and sys.argv[3] == "trace"
W, H, N, T = 1241, 376, 1000, 20
if kind == "scene":
    one = syn.make_sequence(1, w=W, h=H, seed=3, margin=64)[0]
elif kind == "flat":                                  # no lane passes the cardinal test: the early exit everywhere
    one = np.full((1, H, W), 128, np.uint8)
else:                                                 # every wave holds candidates: the arc stage everywhere
    one = np.random.default_rng(0).integers(0, 256, (1, H, W)).astype(np.uint8)
frames = np.ascontiguousarray(np.broadcast_to(one, (B, 1, H, W)))
pts = syn.grid_points(N, W, H, seed=1)
with VoContext(W, H, max_pts=1024, batch=B) as c:
    c.upload_sequence(frames)
    c.points_upload(np.ascontiguousarray(np.broadcast_to(pts, (B, N, 2))))
    c.push_frame_resident(0)
    prms = {"FAST(%d)" % T: c.st_params(fast_threshold=T), "Shi-Tomasi": c.st_params()}
    for rnd in range(ROUNDS):
        for name, prm in prms.items():
            for k in range(WARM):
                c.shi_tomasi_resident(N, 7, prm)
            c.sync()
            if not trace:
                c.profile_enable((c.PROF_ST,))
            for k in range(LAUNCHES):
                c.shi_tomasi_resident(N, 7, prm)
            c.sync()
            n = [len(x) for x in c.shi_tomasi_fetch()] if B > 1 else [len(c.shi_tomasi_fetch())]
            if not trace:
                ms, cnt = c.profile_read(c.PROF_ST)
                c.profile_enable(())
                print("%s B=%d round %d %-10s: detection launch group %8.1f us (%d launches), %d corners in sequence 0" %
                      (kind, B, rnd, name, 1e3 * ms / max(cnt, 1), cnt, n[0]))
