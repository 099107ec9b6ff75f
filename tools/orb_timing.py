"""Time per call of VoContext.orb_detect_compute beside VoContext.sift_detect_compute on the same 1241 x 376 frames, batch 1 and 32, in one
process, and the split of the ORB call over its stages.

Both calls are host-synchronous with their uploads and read-backs: the call a user makes.  Time: hipEvent pairs on the context's stream are what
the stage split uses (vo_profile_enable, regions VO_PROF_ORB_*: the resize launches; score + maxima + cut; Harris + rank; describe) in a loop of
its own, so that the events do not sit in the timed calls; the whole call is timed by the host clock around CALLS calls after WARM warm-up
calls, the two detectors alternating over ROUNDS rounds; median and minimum of the rounds are printed.  Every sequence of a batch gets a
different frame of the synthetic sequence.
usage: tools/orb_timing.py [batch ...]      (default: 1 32)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-odom-pipeline_amd"))
import numpy as np
from vo_mi355x import VoContext, synthetic as syn

ROUNDS, WARM, CALLS = 3, 2, 5
W, H = 1241, 376
frames, _ = syn.make_sequence(8, seed=5)

for B in [int(a) for a in sys.argv[1:]] or [1, 32]:
    imgs = np.stack([frames[b % len(frames)] for b in range(B)]) if B > 1 else frames[0]
    with VoContext(W, H, max_pts=2048, batch=B) as c:
        calls = (("orb_detect_compute", lambda: c.orb_detect_compute(imgs)), ("sift_detect_compute", lambda: c.sift_detect_compute(imgs)))
        times = {name: [] for name, _ in calls}
        last = {}
        for rnd in range(ROUNDS):
            for name, fn in calls:
                for k in range(WARM):
                    fn()
                t0 = time.perf_counter()
                for k in range(CALLS):
                    last[name] = fn()
                times[name].append(1e3 * (time.perf_counter() - t0) / CALLS)
        for name, _ in calls:
            r = last[name] if B > 1 else [last[name]]
            print("B=%2d %-20s: median %8.2f ms, min %8.2f ms per call (%.2f ms per image; %d rounds of %d calls); %d keypoints in sequence 0"
                  % (B, name, np.median(times[name]), min(times[name]), min(times[name]) / B, ROUNDS, CALLS, len(r[0][0])), flush=True)
        print("B=%2d   keypoints per level, sequence 0: %s (quotas %s)" % (B, list(c.orb_levels()["n_l"][0]), list(c.orb_levels()["quota_l"])), flush=True)
        regions = (("pyramid (7 x k_orb_resize)", c.PROF_ORB_PYRAMID), ("candidates (score, nms, cut)", c.PROF_ORB_CANDIDATES),
                   ("retention (harris, rank)", c.PROF_ORB_RETAIN), ("describe", c.PROF_ORB_DESCRIBE))
        c.profile_enable([r for _, r in regions])
        for k in range(CALLS):
            c.orb_detect_compute(imgs)
        total = 0.0
        for name, r in regions:
            ms, cnt = c.profile_read(r)
            total += ms / CALLS
            print("B=%2d   %-30s %8.1f us per call" % (B, name, 1e3 * ms / CALLS), flush=True)
        print("B=%2d   %-30s %8.1f us per call (the rest of a call: uploads, two read-backs of the counters, the outputs)" % (B, "kernels, all stages", 1e3 * total),
              flush=True)
        c.profile_enable(())
