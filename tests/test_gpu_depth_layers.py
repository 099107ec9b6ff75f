"""GPU: the depth filter through the Python layers -- VoContext.depth_seeds / depth_update against the raw C ABI, and Extractor.init_seeds /
update_seeds / seed_landmarks on the rendered sequence against the scene's truth."""
import numpy as np
import pytest

import depth_model as dm
from test_gpu_depth import raw_seed_init, raw_update

pytestmark = pytest.mark.gpu


def test_context_methods_equal_the_raw_abi():
    from vo_mi355x import DepthSeeds, VoContext
    (case,) = [c for c in dm.gpu_cases() if c["name"] == "odd_n65"]
    d = dm.case_data(case)
    img, poses = d["steps"][0]
    with VoContext(*case["size"], max_pts=128) as c:
        c.push_frame(d["ref"])
        rc, seeds, patches, ok = raw_seed_init(c, case["uv"], dm.DEPTH_MEAN, dm.DEPTH_MIN, ref_id=0)
        got = c.depth_seeds(case["uv"], dm.DEPTH_MEAN, dm.DEPTH_MIN)
        assert rc == 0 and isinstance(got, DepthSeeds) and len(got) == len(case["uv"])
        assert got.seeds.tobytes() == seeds[0].tobytes() and got.patches.tobytes() == patches[0].tobytes() and np.array_equal(got.ok, ok[0] != 0)
        assert got.seeds.dtype.itemsize == 56 and got.ok.dtype == bool and not got.ok.all() and np.array_equal(got.diverged, ~got.ok)
        c.push_frame(img)
        s = seeds[0].copy()
        rc, res, match, z, stats = raw_update(c, d["K"], poses, s, patches[0], max_iters=7, px_noise=0.8)
        r2, m2, z2, st2 = c.depth_update(d["K"], poses, got, c.depth_params(max_iters=7, px_noise=0.8))
        assert rc == 0 and got.seeds.tobytes() == s.tobytes()
        assert r2.tobytes() == res[0].tobytes() and m2.tobytes() == match[0].tobytes() and z2.tobytes() == z[0].tobytes()
        assert [st2[k] for k in ("UPDATED", "OUTLIER_NOMATCH", "OUTLIER_ALIGN", "SKIP_INVISIBLE", "SKIP_LONG", "SKIP_DEGENERATE", "SKIP_INACTIVE",
                                 "converged", "diverged")] == stats[0].tolist()
        assert np.array_equal(got.observations, s["flags"] >> 8) and got.observations.max() == 1
        # default parameters
        p = c.depth_params()
        assert (p.max_steps, p.max_iters, p.max_score) == (128, 10, 19200)


def test_extractor_seeds_converge_to_the_scenes_depths():
    """corners of frame 0 as candidates, the true poses in a world that is not camera 0, seven updates: the converged landmarks, moved back
    into the reference camera, are within 3 of their own sigma of the scene's truth at their own pixel (inverse distance along the bearing),
    and what comes back is shaped like triangulate_tracks' output"""
    from vo_mi355x import Extractor, VoContext
    from vo_mi355x.state import Keypoint, Landmark
    sc = dm.scene(dm.W, dm.H)
    K, F = sc["K"], sc["frames"]
    G = np.eye(4)                                    # world -> camera 0
    G[:3, :3], G[:3, 3] = dm.rodrigues([0.1, -0.2, 0.05]), [0.3, -0.1, 2.0]
    Hs = [P @ G for P in sc["poses"]]
    with VoContext(dm.W, dm.H, max_pts=512) as c:
        ext = Extractor(min_kp_dist=7, ctx=c)
        cands = ext.extract(F[0], 0, current_kp=[], detector='shi-tomasi', mask_radius=7, describe=False)
        assert len(cands) >= 60
        with pytest.raises((ValueError, RuntimeError)):
            ext.init_seeds(cands, Hs[0], im_ref=F[0])                           # no prior and no landmarks to take one from
        seeds = ext.init_seeds(cands, Hs[0], depth_mean=dm.DEPTH_MEAN, depth_min=dm.DEPTH_MIN, im_ref=F[0])
        cuv = np.array([k.uv.reshape(2) for k in cands], np.float64)
        # the default prior: the mean and the smallest depth of the given landmarks in the reference camera
        Xl = np.array([[0.5, -0.2, 6.0], [-1.0, 0.3, 9.0], [0.2, 0.1, 12.0], [0.0, 0.0, -4.0]])          # camera 0; the last one is behind it
        Gi = np.linalg.inv(G)
        lms0 = [Landmark(0, (Gi[:3, :3] @ x + Gi[:3, 3]).reshape(3, 1), None) for x in Xl]
        prior = ext.init_seeds(cands, Hs[0], landmarks=lms0, im_ref=F[0])
        assert np.allclose(prior.seeds["mu"], 1.0 / 9.0, rtol=1e-12) and np.allclose(prior.seeds["z_range"], 1.0 / 6.0, rtol=1e-12)
        assert np.allclose(prior.seeds["sigma2"], (1.0 / 6.0) ** 2 / 36.0, rtol=1e-12) and prior.patches.tobytes() == seeds.patches.tobytes()
        half = ext.init_seeds(cands, Hs[0], depth_min=2.0, landmarks=lms0, im_ref=F[0])                 # one of the two given, the other from the landmarks
        assert np.allclose(half.seeds["mu"], 1.0 / 9.0, rtol=1e-12) and (half.seeds["z_range"] == 0.5).all()
        # (a corner within five pixels of the border has no patch: flagged diverged at birth)
        assert len(seeds) == len(cands) and np.array_equal(seeds.ok, dm.scorable(cuv, dm.W, dm.H)) and seeds.ok.sum() >= 60
        with pytest.raises(ValueError):
            ext.seed_landmarks(seeds)                                           # no K yet
        for t in range(1, dm.N_FRAMES):
            res, match, z, st = ext.update_seeds(K, seeds, Hs[t], im_curr=F[t])
            print("frame %d: %s" % (t, st))
        lms, kps, rest = ext.seed_landmarks(seeds, t_curr=dm.N_FRAMES - 1)
        conv = seeds.converged & ~seeds.diverged
        assert len(lms) == len(kps) == int(conv.sum()) >= 30 and len(rest) == len(cands) - len(lms)
        assert all(type(l) is Landmark and l.p.shape == (3, 1) and l.p.dtype == np.float64 and l.t_latest == dm.N_FRAMES - 1 for l in lms)
        assert all(type(k) is Keypoint for k in kps) and [id(k) for k in kps] == [id(cands[i]) for i in np.nonzero(conv)[0]]
        assert all(l.des is k.des for l, k in zip(lms, kps))
        uv = np.array([k.uv.reshape(2) for k in kps], np.float64)
        P = np.array([l.p.reshape(3) for l in lms])
        Xc = P @ G[:3, :3].T + G[:3, 3]
        mu = 1.0 / np.linalg.norm(Xc, axis=1)
        # the landmark lies on its seed's bearing
        assert np.abs(Xc * mu[:, None] - dm.bearing(K, uv)).max() < 1e-9
        err = np.abs(mu - dm.true_mu(sc, uv)) / np.sqrt(seeds.seeds["sigma2"][conv])
        print("%d of %d seeds converged; error in their own sigma: median %.3f, max %.3f" % (len(lms), len(cands), np.median(err), err.max()))
        assert err.max() <= 3.0
        assert np.allclose(seeds.depth_sigma[conv], np.sqrt(seeds.seeds["sigma2"][conv]) / mu ** 2, rtol=1e-9)
        # which="active" and a mask
        assert len(ext.seed_landmarks(seeds, which="active")[0]) == int((~seeds.diverged).sum())
        assert len(ext.seed_landmarks(seeds, which=np.arange(len(cands)) < 5)[0]) == 5
