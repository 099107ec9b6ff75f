"""Cost of CLAHE (vo_set_clahe) forced on at the bench shape: 256 sequences of 1241x376, 8x8 tiles, clip limit 40.

Per-launch time of k_clahe_lut and k_clahe_apply and of the whole frame region from the library's own profile scopes (VO_PROF_CLAHE_LUT,
VO_PROF_CLAHE_APPLY, VO_PROF_FRAME) over pushes of resident frames, then frames/s of the fused front-end step (pyramid, tracker, detector; no
DLT / BA) with the setting off and on, alternating.  Compulsory traffic per step: the raw frames read twice and written once, 3 x 119 MB.
usage: tools/clahe_timing.py [seqs] [image: noise | flat | scene]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-odom-pipeline_amd"))
import numpy as np
from vo_mi355x import VoContext, synthetic as syn
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
kind = sys.argv[2] if len(sys.argv) > 2 else "scene"
W, H, NF, N = 1241, 376, 2, 1000
if kind == "scene":
    one = syn.make_sequence(NF, w=W, h=H, seed=3, margin=64)[0]
elif kind == "flat":                                  # every lane of a wave adds to one bin: the contention worst case
    one = np.full((NF, H, W), 128, np.uint8)
else:
    one = np.random.default_rng(0).integers(0, 256, (NF, H, W)).astype(np.uint8)
frames = np.ascontiguousarray(np.broadcast_to(one, (B, NF, H, W)))
pts = syn.grid_points(N, W, H, seed=1)
with VoContext(W, H, max_pts=1024, batch=B) as c:
    c.upload_sequence(frames)
    c.points_upload(np.ascontiguousarray(np.broadcast_to(pts, (B, N, 2))))
    regions = (c.PROF_FRAME, c.PROF_CLAHE_LUT, c.PROF_CLAHE_APPLY)
    for on in (False, True):
        c.set_clahe(40.0, (8, 8)) if on else c.clear_clahe()
        for k in range(5):
            c.push_frame_resident(k % NF)
        c.profile_enable(regions)
        for k in range(30):
            c.push_frame_resident(k % NF)
        res = [c.profile_read(r) for r in regions]
        c.profile_enable(())
        print("%s B=%d CLAHE %s: frame region %.1f us" % (kind, B, "on " if on else "off", 1e3 * res[0][0] / max(res[0][1], 1)) +
              ("; k_clahe_lut %.1f us, k_clahe_apply %.1f us per launch (%d launches)" %
               (1e3 * res[1][0] / res[1][1], 1e3 * res[2][0] / res[2][1], res[1][1]) if on else ""))
    for rnd in range(3):
        for on in (False, True):
            c.set_clahe(40.0, (8, 8)) if on else c.clear_clahe()
            for k in range(5):
                c.frame_step_resident(k % NF, N, do_dlt=False, do_ba=False); c.frame_fetch()
            t0 = time.perf_counter()
            for k in range(30):
                c.frame_step_resident(k % NF, N, do_dlt=False, do_ba=False); c.frame_fetch()
            dt = (time.perf_counter() - t0) / 30
            print("%s B=%d front-end step, CLAHE %s: %.3f ms per step, %.0f frames/s" % (kind, B, "on " if on else "off", dt * 1e3, B / dt))
