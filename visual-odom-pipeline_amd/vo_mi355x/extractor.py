"""Drop-in for the reference's `Extractor` on the hot path (src/extractor/extractor.py).

Same method names, argument order, defaults, return arities and in-place mutation semantics as the reference
(extend_tracks :38-59, extend_landmarks :61-88, extract :90-132, triangulate_tracks :193-242,
triangulate_nonlinear :244-253, triangulate :255-277), but every OpenCV call is replaced by the HIP library
(VoContext).  Of the bootstrap (reference :114-172) the descriptor matching (match / match_lists) and both RANSAC poses
(camera_pose) and the SIFT detector / descriptor (extract(detector='custom'), cv2.SIFT_create(nfeatures=1000)) run on the
GPU too.
"""
from copy import deepcopy

import numpy as np

from .context import VoContext
from .state import Keypoint, Landmark


class DMatch:
    """the fields of cv2.DMatch the reference reads (queryIdx, trainIdx; extractor.py:147-150, pipeline.py:56-63)"""
    __slots__ = ("queryIdx", "trainIdx", "imgIdx", "distance")

    def __init__(self, queryIdx, trainIdx, distance, imgIdx=0):
        self.queryIdx, self.trainIdx, self.imgIdx, self.distance = int(queryIdx), int(trainIdx), int(imgIdx), float(distance)

    def __repr__(self):
        return "DMatch(queryIdx=%d, trainIdx=%d, distance=%.6g)" % (self.queryIdx, self.trainIdx, self.distance)


class Extractor:
    def __init__(self, cfg=None, min_kp_dist=10, ctx=None, device=0, max_pts=8192, lazy=None, lazy_backend=None, bidir="reference",
                 predict="off", subpix=None, undistort=None, clahe=None, fast_threshold=20, descriptor=None, brief_pattern=None, feature_method='sift',
                 orb_params=None):
        """lazy (default: on unless VO_LAZY=0): once a frame has come through the reference's call order (pipeline.py:98-156) the state moves
        into device tables and the lists this class hands out are views of them (vo_mi355x/lazy.py); lazy_backend: test hook
        (ctx, K, params, width, height) -> backend, default the GPU one.  max_pts: keypoints per call AND the capacity of those tables (<= 8192).
        bidir: what a finite max_bidir_error of extend_tracks / extend_landmarks means.  "reference" (default): the reference's check, whose
        second KLT call tracks FORWARD again from p1 (extractor.py:45,66).  "backward": the true forward-backward check,
        LK(cur, prev, p1) as in the OpenCV sample the reference copies (notebooks/tracking.py:39-42), both passes in one vo_klt_track_fb
        launch; a keypoint whose round trip misses its start by max_bidir_error or more (max over x, y; float32) is dropped / goes to the dead
        lists like one outside the image.  max_bidir_error = inf is the plain path in both modes.  A lazy session serves only the infinite
        threshold: a call with a finite one takes the plain path (the session ends there), as it always has.
        predict: where extend_tracks / extend_landmarks start the tracker.  "off" (default): at k.uv, the reference's flags = 0 call
        (extractor.py:44,65).  "constant_velocity": at g = uv + (uv - k.uv_history[-2]) in float32 (g = uv for a history of fewer than two
        entries), OpenCV's OPTFLOW_USE_INITIAL_FLOW through VoContext.klt_track(init=g); the second pass of either bidir mode is not seeded.
        A lazy session serves only "off": with a prediction every call takes the plain path.
        subpix: None (default): extract(detector='shi-tomasi') hands out the detector's integer corners, as the reference does
        (extractor.py:111).  dict(win=(5, 5), zero_zone=(-1, -1), criteria=(3, 40, 0.001)) -- cv2.cornerSubPix's arguments, any key may be
        left out: the corners are refined against the image they were detected on (VoContext.corner_subpix), and the new keypoints' uv,
        uv_first and uv_history[0] are the refined positions.  A lazy session serves only None: with refinement every call takes the
        plain path.
        undistort: None (default): images are tracked as given.  dict(K=, dist=[, new_K=]) -- cv2.undistort's arguments: the setting goes to
        this extractor's context (VoContext.set_undistort), so _im_prev and im_curr enter the frame store undistorted and extend_tracks /
        extend_landmarks / extract work in the undistorted camera.  A lazy session serves only None.
        clahe: None (default): images are tracked as given.  (clip_limit, (tiles_x, tiles_y)) -- cv2.createCLAHE's arguments: the setting goes
        to this extractor's context (VoContext.set_clahe), so _im_prev and im_curr enter the frame store equalised (behind the undistortion).
        A lazy session serves only None.
        fast_threshold: the threshold of extract(detector='fast') (self._fast_params, cv2.FastFeatureDetector_create's arguments): the FAST-9/16
        score is ranked in place of the Shi-Tomasi response; maxCorners, qualityLevel and minDistance still come from _shitomasi_params.
        A lazy session does not serve that detector: such a call takes the plain path.
        descriptor: None (default): extract(detector='shi-tomasi' | 'fast', describe=True) raises NotImplementedError -- a corner has no SIFT
        scale.  'brief': such a call describes the detector's integer corners with the oriented BRIEF descriptor (VoContext.brief_compute;
        the reference's cv2.ORB_create() branch, extractor.py:30-31, 119-122) and returns Keypoints whose `des` is the (32, 1) uint8 column;
        corners within 24 pixels of a border are dropped, as cv2.ORB.compute drops border keypoints.  brief_pattern: 256 rows
        (x1, y1, x2, y2) in [-15, 15], None = the default table.  match / match_lists on uint8 descriptors take the reference's 'orb' branch
        (1-NN under the Hamming distance, extractor.py:144-145).  A lazy session does not describe: such a call takes the plain path.
        feature_method: what extract(detector='custom') runs, the reference's two feature methods (extractor.py:26-33).  'sift' (default):
        cv2.SIFT_create(nfeatures=1000).  'orb': the multi-scale ORB detector (VoContext.orb_detect_compute; cv2.ORB_create()'s defaults
        nfeatures=500, scaleFactor=1.2, nlevels=8, fastThreshold=20, any of them replaced through orb_params=dict(...)): Keypoints at (x, y) of
        the input image whose `des`, with describe=True, is the (32, 1) uint8 column; brief_pattern is its sampling table too."""
        if feature_method not in ('sift', 'orb'):
            raise ValueError("feature_method must be 'sift' or 'orb'")
        self._feature_method = feature_method
        unknown = set(orb_params or {}) - {"nfeatures", "scale_factor", "nlevels", "fast_threshold"}
        if unknown:
            raise ValueError("orb_params: unknown keys %r" % sorted(unknown))
        self._orb_params = dict(orb_params or {})
        if descriptor not in (None, 'brief'):
            raise ValueError("descriptor must be None or 'brief'")
        self._descriptor = descriptor
        self._brief_pattern = None if brief_pattern is None else VoContext._brief_pattern(brief_pattern)
        if clahe is not None:
            clip, tx, ty = VoContext._clahe_args(clahe)
            clahe = (clip, (tx, ty))
        self._clahe = clahe
        if undistort is not None:
            VoContext._undistort_args(undistort)
        self._undistort = None if undistort is None else dict(undistort)
        if subpix is not None:
            unknown = set(subpix) - {"win", "zero_zone", "criteria"}
            if unknown:
                raise ValueError("subpix: unknown keys %r" % sorted(unknown))
        self._subpix = None if subpix is None else dict(subpix)
        if bidir not in ("reference", "backward"):
            raise ValueError("bidir must be 'reference' or 'backward'")
        if predict not in ("off", "constant_velocity"):
            raise ValueError("predict must be 'off' or 'constant_velocity'")
        self._bidir = bidir
        self._predict = predict
        from . import lazy as _lz
        self._cfg = cfg
        self._lazy_on = _lz.enabled() if lazy is None else bool(lazy)
        self._lazy_backend = lazy_backend
        self._lazy = None               # the live session, if any
        self._trace = []                # the plain-path calls of the current frame, in order (is this the reference's Pipeline.step?)
        self._seen = {}                 # parameters those calls came with (a session is created with them)
        _lz._EXTRACTORS.add(self)
        # parameters hard-coded by the reference (extractor.py:16-24)
        self._lk_params = dict(winSize=(31, 31), maxLevel=3, criteria=(3, 30, 0.03))
        self._shitomasi_params = dict(maxCorners=1000, qualityLevel=0.03, minDistance=min_kp_dist, blockSize=31)
        self._fast_params = dict(threshold=int(fast_threshold), nonmaxSuppression=True)
        self._ctx = ctx
        self._device, self._max_pts = device, max_pts
        self._im_prev = None            # set by the caller, exactly like the reference (pipeline.py:36,103)
        self._dev_prev = None           # host copies of what the device frame store currently holds
        self._dev_cur = None
        if ctx is not None:
            self._apply_ingest(ctx)

    # -- device frame store ---------------------------------------------------------------------
    def _context(self, img):
        if self._ctx is None:
            h, w = img.shape
            self._ctx = VoContext(w, h, max_pts=self._max_pts, device=self._device,
                                  max_level=self._lk_params["maxLevel"], win=self._lk_params["winSize"][0])
            self._apply_ingest(self._ctx)
        return self._ctx

    def _apply_ingest(self, ctx):
        """the settings (undistort=, clahe=) go to the context the frames are pushed to; None makes no call at all (a caller's context keeps
        what it has, and a stand-in context needs no such method)"""
        if self._undistort is not None or self._clahe is not None:
            ctx.apply_ingest(self._undistort, self._clahe, clear_missing=False)

    def _push(self, img):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        self._context(img).push_frame(img)
        self._dev_prev, self._dev_cur = self._dev_cur, img.copy()

    @staticmethod
    def _same(a, b):
        return a is not None and b is not None and a.shape == b.shape and np.array_equal(a, b)

    def _ensure_pair(self, im_prev, im_curr):
        """make (prev, cur) on the device equal (im_prev, im_curr) with as few uploads as possible"""
        if self._same(self._dev_prev, im_prev) and self._same(self._dev_cur, im_curr):
            return
        if not self._same(self._dev_cur, im_prev):
            self._push(im_prev)
        self._push(im_curr)

    def _ensure_cur(self, img):
        if not self._same(self._dev_cur, img):
            self._push(img)

    def _klt_prm(self):
        return self._ctx.klt_params(win=self._lk_params["winSize"][0], max_level=self._lk_params["maxLevel"],
                                    max_count=self._lk_params["criteria"][1], epsilon=self._lk_params["criteria"][2])

    def _klt(self, p0, init=None):
        if init is None:
            return self._ctx.klt_track(p0, self._klt_prm())
        return self._ctx.klt_track(p0, self._klt_prm(), init=init)

    def _guess(self, kps, p0):
        """predict="constant_velocity": the start positions (n, 2) float32 of a keypoint list whose positions are p0; else None"""
        if self._predict == "off":
            return None
        g = p0.copy()
        for i, k in enumerate(kps):
            if len(k.uv_history) >= 2:
                prev = np.asarray(k.uv_history[-2], np.float64).reshape(2).astype(np.float32)
                g[i] = p0[i] + (p0[i] - prev)
        return g

    def _track(self, im_curr, p0, max_bidir_error, init=None):
        """p1 and the 'bidirectional' flag.  bidir="reference": the reference's second pass tracks FORWARD again from
        p1 (extractor.py:45,66); with an infinite threshold its result cannot change `good` (NaN aside), so it
        is skipped then.  bidir="backward" with a finite threshold: the forward-backward check (vo_klt_track_fb)."""
        self._ensure_pair(self._im_prev, im_curr)
        if self._bidir == "backward" and max_bidir_error != np.inf:
            c = self._ctx
            p1, _st, _err, _p0r, fb_err = c.klt_track_fb(p0, self._klt_prm(), **({} if init is None else dict(init=init)))
            return p1, fb_err < np.float32(max_bidir_error)
        p1, _st, _err = self._klt(p0, init)
        if np.isinf(max_bidir_error):
            good = ~np.isnan(p1).any(axis=1)
        else:
            p0r, _st, _err = self._klt(p1)
            good = np.abs(p0 - p0r).max(-1) < max_bidir_error
        return p1, good

    # -- the lazy boundary (lazy.py) ---------------------------------------------------------------
    def _session(self):
        s = self._lazy
        if s is not None and not s.alive:
            s = self._lazy = None
        return s

    def _plain(self, name, img=None, **seen):
        """a call is about to take the plain path: a live session ends here (its proxies become plain objects first), and the call is noted"""
        s = self._session()
        if s is not None:
            s.desync("%s took the plain path" % name)
            self._lazy = None
        if name == "extend_tracks":
            self._trace = []
        self._trace.append((name, None if img is None else id(img)))
        self._seen.update(seen)

    def _frame_is_reference_order(self):
        """extend_tracks, extend_landmarks, camera_pose('3D-2D'), triangulate_tracks -- each once, in this order, on one image"""
        names = [n for n, _ in self._trace]
        imgs = {i for n, i in self._trace[:2]}
        return names == ["extend_tracks", "extend_landmarks", "camera_pose", "triangulate_tracks"] and len(imgs) == 1

    def _fast_pushed(self, s):
        """the session pushed a frame into the context's store: keep this class's record of the store's contents"""
        if self._dev_cur is not s.cur_img:
            self._dev_prev, self._dev_cur = self._dev_cur, s.cur_img

    # -- KLT ------------------------------------------------------------------------------------
    def _survivors(self, im_curr, p1, good):
        """keep mask of the reference's rule (0 <= x <= W and 0 <= y <= H, ends included, and the 'bidirectional' flag)
        plus two independent (n, 2, 1) float32 blocks whose rows become k.uv and the new history entry -- one allocation
        each instead of two small arrays per keypoint; every keypoint still owns its own values (separate rows, and the
        history entry is not the same memory as uv, exactly like the reference's two np.array(...) calls)."""
        h, w = im_curr.shape[0], im_curr.shape[1]
        keep = good & (p1[:, 0] >= 0) & (p1[:, 0] <= w) & (p1[:, 1] >= 0) & (p1[:, 1] <= h)
        uv = p1.reshape(-1, 2, 1).copy()
        return keep, uv, uv.copy()

    def _start(self, init, kps, p0):
        """where the tracker starts: `init` (n, 2), e.g. project_landmarks under align_frame's pose, in place of this class's own guess"""
        if init is None:
            return self._guess(kps, p0)
        g = np.ascontiguousarray(init, np.float32).reshape(-1, 2)
        if g.shape != p0.shape:
            raise ValueError("init must hold one start position per keypoint")
        return g

    def extend_tracks(self, im_curr, kp, max_bidir_error=30, init=None):
        """init (None: as the reference): start positions (len(kp), 2) for the tracker in place of predict='s guess; a call with it takes
        the plain path, like every call a lazy session does not serve"""
        s = self._session() if init is None else None
        if s is not None:
            r = s.extend_tracks(self._im_prev, im_curr, kp, max_bidir_error)
            if r is not NotImplemented:
                self._fast_pushed(s)
                return r
        self._plain("extend_tracks", im_curr, max_bidir_error=max_bidir_error)
        new_tracks = []
        if len(kp):
            p0 = self._uv_block(kp)
            p1, good = self._track(im_curr, p0, max_bidir_error, self._start(init, kp, p0))
            keep, uv, hist = self._survivors(im_curr, p1, good)
            for i in np.nonzero(keep)[0]:
                k = kp[i]
                k.uv = uv[i]
                k.t_total += 1
                k.uv_history.append(hist[i])
                new_tracks.append(k)
        return new_tracks

    def extend_landmarks(self, im_curr, landmarks, landmarks_kp, max_bidir_error=30, init=None):
        """init: as extend_tracks, one start position per landmark keypoint"""
        s = self._session() if init is None else None
        if s is not None:
            r = s.extend_landmarks(self._im_prev, im_curr, landmarks, landmarks_kp, max_bidir_error)
            if r is not NotImplemented:
                self._fast_pushed(s)
                return r
        self._plain("extend_landmarks", im_curr)
        landmarks_new, kp_new, landmarks_dead, kp_dead = [], [], [], []
        if not len(landmarks_kp):
            return landmarks_new, kp_new, landmarks_dead, kp_dead
        p0 = self._uv_block(landmarks_kp)
        p1, good = self._track(im_curr, p0, max_bidir_error, self._start(init, landmarks_kp, p0))
        keep, uv, hist = self._survivors(im_curr, p1, good)
        # the reference converts p1 with .tolist() here (python floats): uv / history entries are float64 in this method
        uv, hist = uv.astype(np.float64), hist.astype(np.float64)
        for i in range(len(landmarks)):
            l, k = landmarks[i], landmarks_kp[i]
            if not keep[i]:
                landmarks_dead.append(l)
                kp_dead.append(k)
                continue
            k.uv = uv[i]
            k.t_total += 1
            k.uv_history.append(hist[i])
            l.t_latest += 1
            kp_new.append(deepcopy(k))
            landmarks_new.append(l)
        return landmarks_new, kp_new, landmarks_dead, kp_dead

    # -- re-detection ---------------------------------------------------------------------------
    def extract(self, img, t, current_kp=[], detector='custom', mask_radius=5, describe=False):
        if detector == 'custom':
            if self._feature_method == 'orb':
                self._plain("extract_orb")
                return self._extract_orb(img, t, current_kp, describe)
            self._plain("extract_sift")
            return self._extract_sift(img, t, current_kp, describe)
        if detector not in ('shi-tomasi', 'fast'):
            raise ValueError("detector must be 'shi-tomasi', 'fast' or 'custom'")
        if describe and self._descriptor != 'brief':
            raise NotImplementedError("describe=True needs detector='custom' (SIFT): a Shi-Tomasi or FAST corner has no SIFT scale")
        fast = detector == 'fast'
        if fast and not self._fast_params.get("nonmaxSuppression", True):
            raise NotImplementedError("detector='fast' ranks 3 x 3 maxima of the score: nonmaxSuppression=False is not served")
        s = self._session()
        if s is not None:
            if describe:
                r = s.extract(img, t, current_kp, mask_radius, detector=detector, describe=True)
            else:
                r = s.extract(img, t, current_kp, mask_radius, detector=detector) if fast else s.extract(img, t, current_kp, mask_radius)
            if r is not NotImplemented:
                return r
        self._plain("extract", mask_radius=mask_radius)
        self._context(img)
        self._ensure_cur(img)
        c = self._ctx
        sp = self._shitomasi_params
        # the dict is what the reference splats into cv2.goodFeaturesToTrack (extractor.py:111); its optional keys are honoured too
        prm = c.st_params(max_corners=sp["maxCorners"], quality_level=sp["qualityLevel"],
                          min_distance=sp["minDistance"], block_size=sp["blockSize"],
                          use_harris=bool(sp.get("useHarrisDetector", False)), harris_k=sp.get("k", 0.04))
        if fast:                             # the FAST-9/16 score in place of the response; the selection keys above stay in force
            prm = c.st_params(max_corners=sp["maxCorners"], quality_level=sp["qualityLevel"], min_distance=sp["minDistance"],
                              block_size=sp["blockSize"], fast_threshold=self._fast_params["threshold"])
        # np.int32(kp.uv) truncation happens on the device; float32 carries every pixel coordinate exactly
        cur = (np.array([k.uv for k in current_kp], dtype=np.float64).reshape(-1, 2).astype(np.float32) if len(current_kp)
               else np.zeros((0, 2), np.float32))
        kp = c.shi_tomasi(cur if len(cur) else None, mask_radius=mask_radius, params=prm)
        if kp.shape[0] == 0:
            return []
        desc = None
        if describe:                         # self._features.compute(img, cv_kp) on the integer corners; border keypoints leave the list
            desc, _angle, flags = c.brief_compute(kp, "cur", pattern=self._brief_pattern)
            kp, desc = np.ascontiguousarray(kp[flags == 0]), np.ascontiguousarray(desc[flags == 0]).reshape(-1, 32, 1)
            if kp.shape[0] == 0:
                return []
        if self._subpix is not None:         # cv2.cornerSubPix(img, kp, win, zero_zone, criteria) on the image just detected on
            crit = self._subpix.get("criteria", (3, 40, 0.001))
            kp = c.corner_subpix(kp, "cur", c.subpix_params(win=self._subpix.get("win", (5, 5)), zero_zone=self._subpix.get("zero_zone", (-1, -1)),
                                                            max_count=crit[1], epsilon=crit[2]))
        # like the reference (extractor.py:127-131) uv_first, uv and the first history entry of a new keypoint are three
        # VIEWS of the same row of the detector output (kp[i, :].reshape((2, 1)) is a view); des a view of the zero column
        kp3 = kp.reshape(-1, 2, 1)
        if desc is None:
            desc = np.zeros((kp.shape[0], 1, 1))
        return [Keypoint(t_first=t, t_total=1, uv_first=kp3[i], uv=kp3[i], des=desc[i], uv_history=[kp3[i]])
                for i in range(len(kp))]

    # -- triangulation --------------------------------------------------------------------------
    @staticmethod
    def _uv_block(kps):
        """(n, 2) float32 pixel coordinates of a keypoint list: one float64 gather, one rounding to float32 (the reference
        rounds its stacked (n, 1, 2) array the same way before cv2.triangulatePoints, extractor.py:264-265)"""
        return np.asarray([k.uv for k in kps], dtype=np.float64).reshape(-1, 2).astype(np.float32)

    def _two_view(self, K, H0, H1, keyp0, keyp1, want_stats):
        """k_dlt for one view pair -> (points [n, 3] float32, camera-1 depth, mean reprojection error).  The projection matrices
        are rounded to float32 before the solve, as the reference hands them to OpenCV (extractor.py:268-269)."""
        if self._ctx is None:
            raise RuntimeError("Extractor: no device context yet (track or extract a frame first, or pass ctx=)")
        cams = [np.float32(np.asarray(K) @ np.asarray(H)[:3]) for H in (H0, H1)]
        pix = [self._uv_block(keyp0), self._uv_block(keyp1)]
        if want_stats:
            X4, depth1, reproj = self._ctx.triangulate(cams[0], cams[1], pix[0], pix[1], K, H0, H1)
        else:
            X4, depth1, reproj = self._ctx.triangulate(cams[0], cams[1], pix[0], pix[1]), None, None
        X4 = X4.reshape(4, -1)
        return (X4[:3] / X4[3]).T, depth1, reproj            # float32 division, point by point

    @staticmethod
    def _as_landmarks(points, rows, kps, t):
        """Landmark(t, p (3, 1) float64 holding the float32 values, des of the view-1 keypoint)"""
        wide = np.asarray(points, np.float64)
        return [Landmark(t, wide[i].reshape(3, 1).copy(), kps[i].des) for i in rows]

    def triangulate(self, K, H0, H1, keyp0, keyp1, t):
        if not len(keyp0):
            return []
        pts, _, _ = self._two_view(K, H0, H1, keyp0, keyp1, False)
        return self._as_landmarks(pts, range(len(pts)), keyp1, t)

    def triangulate_nonlinear(self, K, H0, H1, keyp0, keyp1, t, max_err_reproj=1.0):
        """DLT + the filters of TriangulatorNL.refine (triangulate.py:82-146): camera-1 cheirality, then mean
        reprojection error < max_err_reproj.  The reference's scipy "refinement" never moves a point (its
        sparsity pattern is empty for the keypoint columns) and its final filter repeats the
        second one, so the result is exactly these two filters; like the reference, the surviving keypoints'
        `uv` come back as float64 (2,1) arrays."""
        if not len(keyp0):
            return [], [], []
        pts, depth1, reproj = self._two_view(K, H0, H1, keyp0, keyp1, True)
        rows = np.nonzero((np.asarray(depth1) > 0) & (np.asarray(reproj) < max_err_reproj))[0]
        for view in (keyp0, keyp1):
            for i in rows:
                view[i].uv = np.array(view[i].uv, dtype=np.float64).reshape(2, 1)
        return self._as_landmarks(pts, rows, keyp1, t), [keyp0[i] for i in rows], [keyp1[i] for i in rows]

    @staticmethod
    def _group_gate(H_birth, H_now, p_first, min_angle_deg):
        """The reference's per-group "bearing angle" test (extractor.py:231-240), which is not a bearing angle: the triangle
        side `a` is the FROBENIUS NORM of the 4x4 relative transform (>= 2), the other two sides are the lengths of the
        group's FIRST landmark rotated into either camera as a direction (w = 0, so both equal |p|).  Law of cosines,
        degrees; NaN (|cos| > 1) rejects.  In effect: accept the whole group iff |p_first| is large enough against a."""
        ray = np.zeros(4)
        ray[:3] = np.asarray(p_first, np.float64).ravel()
        a = np.linalg.norm(np.asarray(H_now) @ np.linalg.inv(H_birth))
        b, c = np.linalg.norm(np.asarray(H_birth) @ ray), np.linalg.norm(np.asarray(H_now) @ ray)
        with np.errstate(invalid='ignore', divide='ignore'):
            theta = np.degrees(np.arccos((b * b + c * c - a * a) / (2 * b * c)))
        return bool(theta > min_angle_deg)                   # False for NaN

    def triangulate_tracks(self, K, candidates_kp, trajectory, t_curr, refine=True, min_track_length=5,
                           min_bearing_angle=10, max_err_reproj=4.0):
        """Candidates that reached `min_track_length` leave the candidate list (triangulated or not); they are triangulated
        per birth frame between their first and their newest observation and a group is kept iff its gate passes
        (reference extractor.py:193-242).  -> (new landmarks, their keypoints, remaining candidates)"""
        s = self._session()
        if s is not None and refine:
            r = s.triangulate_tracks(K, candidates_kp, trajectory, t_curr, min_track_length, min_bearing_angle, max_err_reproj)
            if r is not NotImplemented:
                return r
        self._plain("triangulate_tracks", min_track_length=min_track_length, min_bearing_angle=min_bearing_angle, tri_max_err=max_err_reproj)
        ripe = [k for k in candidates_kp if k.t_total >= min_track_length]
        waiting = [k for k in candidates_kp if k.t_total < min_track_length]
        out_l, out_k = [], []
        if not ripe:
            return out_l, out_k, waiting
        by_birth = {}
        for k in ripe:
            by_birth.setdefault(k.t_first, []).append(k)
        H_now = trajectory[len(trajectory) - 1]
        # the reference walks a SET of birth frames built from the ripe list; building it the same way gives the same
        # iteration order, which is the order of the returned lists
        for born in set(k.t_first for k in ripe):
            newest = by_birth[born]
            # view-0 stand-ins: only `uv` (:= the first observation) is read and rewritten downstream
            oldest = [Keypoint(k.t_first, k.t_total, k.uv_first, np.array(k.uv_first), k.des, []) for k in newest]
            H_birth = trajectory[born]
            lms, _, kept = self.triangulate_nonlinear(K, H_birth, H_now, oldest, newest, t_curr, max_err_reproj=max_err_reproj)
            if lms and self._group_gate(H_birth, H_now, lms[0].p, min_bearing_angle):
                out_l.extend(lms)
                out_k.extend(kept)
        return out_l, out_k, waiting

    def _extract_sift(self, img, t, current_kp, describe):
        """detector='custom' (reference extractor.py:114-131): cv2.SIFT_create(nfeatures=1000).detect(img, mask) and,
        with describe=True, .compute(img, kps) -> Keypoints whose `des` is the (128, 1) float32 descriptor column
        (a (1, 1) zero column without describe).  The bootstrap calls it with no current keypoints (pipeline.py:48-49)."""
        if len(current_kp):
            raise NotImplementedError("SIFT detection with a keypoint mask is not used by the reference pipeline")
        self._context(img)
        kps, desc = self._ctx.sift_detect_compute(img, nfeatures=1000)
        kp = np.ascontiguousarray(kps[:, :2], np.float32)          # cv2.KeyPoint_convert: (n, 2) float32
        if not describe:
            desc = np.zeros((kp.shape[0], 1))
        return [Keypoint(t_first=t, t_total=1, uv_first=kp[i, :].reshape((2, 1)), uv=kp[i, :].reshape((2, 1)),
                         des=desc[i, :].reshape((-1, 1)), uv_history=[kp[i, :].reshape((2, 1))]) for i in range(len(kp))]

    def _extract_orb(self, img, t, current_kp, describe):
        """detector='custom' with feature_method='orb' (reference extractor.py:30-31, 114-131): cv2.ORB_create().detect(img, mask) and, with
        describe=True, .compute(img, kps) -> Keypoints whose `des` is the (32, 1) uint8 descriptor column (a (1, 1) zero column without)."""
        if len(current_kp):
            raise NotImplementedError("ORB detection with a keypoint mask is not used by the reference pipeline")
        self._context(img)
        kps, desc = self._ctx.orb_detect_compute(img, pattern=self._brief_pattern, **self._orb_params)
        kp = np.ascontiguousarray(np.stack([kps["x"], kps["y"]], axis=1), np.float32).reshape(-1, 2)
        if not describe:
            desc = np.zeros((kp.shape[0], 1))
        return [Keypoint(t_first=t, t_total=1, uv_first=kp[i, :].reshape((2, 1)), uv=kp[i, :].reshape((2, 1)),
                         des=desc[i, :].reshape((-1, 1)), uv_history=[kp[i, :].reshape((2, 1))]) for i in range(len(kp))]

    # -- bootstrap (reference extractor.py:134-191) -------------------------------------------------
    _feature_method = 'sift'
    _sift_ratio = 0.80                                   # reference extractor.py:29

    def match(self, desc_1, desc_2):
        """cv2.BFMatcher().knnMatch(desc_1, desc_2, k=2) + Lowe's ratio test (reference extractor.py:134-145): the
        list of DMatch whose nearest neighbour is closer than _sift_ratio x the second nearest.  uint8 descriptors (descriptor='brief'):
        one DMatch per query, its nearest train row under the Hamming distance."""
        if self._ctx is None:
            raise RuntimeError("match needs the device context: track a frame first (or pass ctx=)")
        if np.asarray(desc_1).dtype == np.uint8 and np.asarray(desc_2).dtype == np.uint8:
            # binary descriptors: the reference's 'orb' branch, self._matcher.match(desc_1, desc_2) (extractor.py:144-145) -- the nearest train
            # row of every query under the Hamming distance, no ratio test
            if len(desc_1) == 0 or len(desc_2) == 0:
                return []
            idx, dist = self._ctx.match_hamming_knn2(desc_1, desc_2)
            return [DMatch(q, idx[q, 0], dist[q, 0]) for q in range(len(desc_1))]
        desc_1 = np.ascontiguousarray(desc_1, np.float32); desc_2 = np.ascontiguousarray(desc_2, np.float32)
        if len(desc_2) < 2:
            raise ValueError("not enough values to unpack (expected 2, got %d)" % len(desc_2))   # the reference's `for m, n in matches`
        idx, dist = self._ctx.match_knn2(desc_1, desc_2)
        good = []
        for q in range(len(desc_1)):
            m_d, n_d = float(dist[q, 0]), float(dist[q, 1])
            if m_d < self._sift_ratio * n_d:
                good.append(DMatch(q, idx[q, 0], m_d))
        return good

    def match_lists(self, list_1, list_2):
        """ratio-test matches between two lists of keypoints / landmarks by their `des` columns (reference
        extractor.py:147-154): m.queryIdx indexes list_1, m.trainIdx list_2"""
        rows = [np.stack([np.ravel(o.des) for o in lst]) for lst in (list_1, list_2)]
        return self.match(rows[0], rows[1])

    def match_guided(self, list_1, list_2, F=None, centers=None, **kw):
        """the second matching pass between two lists of objects with `.uv` and `.des` (keypoints, landmarks): VoContext.match_guided over
        their descriptor rows and positions -> the list of DMatch of the accepted queries (m.queryIdx indexes list_1, m.trainIdx list_2).
        F (3,3) with epi_dist=, or centers (n1,2) / the queries' own positions with radius=, narrow the search; ratio=, max_dist= and
        cross_check= as VoContext.match_guided.  Float descriptors take the L2 kernel, uint8 ones the Hamming kernel."""
        if self._ctx is None:
            raise RuntimeError("match_guided needs the device context: track a frame first (or pass ctx=)")
        if len(list_1) == 0 or len(list_2) == 0:
            return []
        rows = [np.stack([np.ravel(o.des) for o in lst]) for lst in (list_1, list_2)]
        if not (rows[0].dtype == np.uint8 and rows[1].dtype == np.uint8):
            rows = [np.ascontiguousarray(r, np.float32) for r in rows]
        p1, p2 = self._uv_pairs(list_1, list_2)
        r = self._ctx.match_guided(rows[0], rows[1], pts1=p1, pts2=p2, F=F, centers=centers, **kw)
        return [DMatch(q, int(j), r["dist"][q, 0]) for q, j in enumerate(r["match"]) if j >= 0]

    def match_list(self, kp_1, desc_1, keypoints):
        # the reference's match_list (extractor.py:156-160) calls self.match with four arguments and always raises
        raise TypeError("match() takes 3 positional arguments but 5 were given")

    def camera_pose(self, K, list_1, list_2, corr='2D-2D', max_err_reproj=4.0):
        """Pose from correspondences -> (inlier indices as a list, H 4x4).
        corr='3D-2D' (reference extractor.py:174-191): cv2.solvePnPRansac(..., reprojectionError=max_err_reproj,
        iterationsCount=1e6, confidence=0.9999) + Rodrigues; H maps world -> camera.
        corr='2D-2D' (reference extractor.py:162-172, the bootstrap): cv2.findEssentialMat(prob=0.9999, RANSAC,
        threshold=1.0) + cv2.recoverPose on its inliers; H maps view-1 -> view-2 coordinates, |t| = 1.
        RANSAC draws differ from OpenCV's (statistical parity, see include/vo_mi355x.h)."""
        if corr == '3D-2D':
            s = self._session()
            if s is not None:
                r = s.camera_pose(K, list_1, list_2, max_err_reproj)
                if r is not NotImplemented:
                    return r
        self._plain("camera_pose" if corr == '3D-2D' else "camera_pose_2d2d", pose_max_err=max_err_reproj)
        if self._ctx is None:
            raise RuntimeError("camera_pose needs the device context: track a frame first (or pass ctx=)")
        if corr == '2D-2D':
            kp_1_pts = np.array([kp.uv.T for kp in list_1]).astype(np.float32).reshape(-1, 2)
            kp_2_pts = np.array([kp.uv.T for kp in list_2]).astype(np.float32).reshape(-1, 2)
            _E, R, t, inliers, st = self._ctx.essential_ransac(np.asarray(K, np.float64), kp_1_pts, kp_2_pts, threshold=1.0,
                                                               prob=0.9999)
            if st["status"] != 0:
                raise RuntimeError("findEssentialMat found no model")     # cv2 returns E = None -> the reference crashes in recoverPose
            H = np.eye(4)
            H[:3, :3] = R
            H[:3, 3] = t.reshape((3,))
            return inliers.reshape((-1,)).tolist(), H
        if corr != '3D-2D':
            raise ValueError("corr must be '2D-2D' or '3D-2D'")
        from .so3 import rodrigues_vec_to_mat
        pts3d = np.array([kp.p.T for kp in list_1]).astype(np.float32).reshape(-1, 3)
        pts2d = np.array([kp.uv.T for kp in list_2]).astype(np.float32).reshape(-1, 2)
        rvec, t, inliers, st = self._ctx.pnp_ransac(np.asarray(K, np.float64), pts3d, pts2d, reproj_err=max_err_reproj,
                                                    confidence=0.9999, max_iters=1000000)
        if st["status"] != 0:
            raise RuntimeError("solvePnPRansac found no pose")          # cv2 returns retval False and inliers None -> the reference crashes too
        H = np.eye(4)
        H[:3, :3] = rodrigues_vec_to_mat(rvec)
        H[:3, 3] = t.reshape((3,))
        return inliers.reshape((-1,)).tolist(), H

    def _uv_pairs(self, list_1, list_2):
        return tuple(np.array([kp.uv.T for kp in lst]).astype(np.float32).reshape(-1, 2) for lst in (list_1, list_2))

    def find_homography(self, list_1, list_2, **kw):
        """cv2.findHomography(RANSAC) between the `uv` of two lists of keypoints (the lists camera_pose takes; the model the reference's
        bootstrap names at pipeline.py:66 and never fits) -> (H 3x3 with x2 ~ H x1 and h33 = 1, inlier indices as a list, stats dict, H0);
        keywords as VoContext.find_homography"""
        if self._ctx is None:
            raise RuntimeError("find_homography needs the device context: track a frame first (or pass ctx=)")
        H, inliers, st, H0 = self._ctx.find_homography(*self._uv_pairs(list_1, list_2), **kw)
        return H, inliers.reshape((-1,)).tolist(), st, H0

    def find_fundamental(self, list_1, list_2, **kw):
        """cv2.findFundamentalMat(FM_RANSAC) between the `uv` of two lists of keypoints (the lists camera_pose takes): the epipolar
        verification of matches that needs no K -> (F 3x3 with x2^T F x1 = 0 and f33 = 1, inlier indices as a list, stats dict, F0);
        keywords as VoContext.find_fundamental"""
        if self._ctx is None:
            raise RuntimeError("find_fundamental needs the device context: track a frame first (or pass ctx=)")
        F, inliers, st, F0 = self._ctx.find_fundamental(*self._uv_pairs(list_1, list_2), **kw)
        return F, inliers.reshape((-1,)).tolist(), st, F0

    def align_landmarks(self, list_1, list_2, matches=None, **kw):
        """The similarity between two maps through the landmarks both hold -- what joins a map that bootstrap_pose has started anew, with
        its own scale and origin, to the old one.  list_1, list_2: lists of Landmark; matches: DMatch es as match_lists returns them
        (m.queryIdx indexes list_1, m.trainIdx list_2), wrong ones among them allowed; None: the lists are index-aligned.
        -> (S 4x4 with p_2 ~ S p_1 in homogeneous coordinates, S[:3, :3] = s R; the indices of the inlier pairs -- into `matches`, or into
        the lists -- as a list; stats dict); keywords as VoContext.estimate_sim3"""
        if self._ctx is None:
            raise RuntimeError("align_landmarks needs the device context: track a frame first (or pass ctx=)")
        if matches is None:
            pairs = [(i, i) for i in range(min(len(list_1), len(list_2)))]
        else:
            pairs = [(m.queryIdx, m.trainIdx) for m in matches]
        src = np.array([np.asarray(list_1[i].p, np.float64).reshape(3) for i, _ in pairs], np.float32).reshape(-1, 3)
        dst = np.array([np.asarray(list_2[j].p, np.float64).reshape(3) for _, j in pairs], np.float32).reshape(-1, 3)
        s, R, t, inliers, st, _ = self._ctx.estimate_sim3(src, dst, **kw)
        S = np.eye(4)
        S[:3, :3], S[:3, 3] = s * R, t
        return S, inliers.reshape((-1,)).tolist(), st

    @staticmethod
    def _points_in_camera(H, landmarks):
        """the landmarks' world points in the camera of pose H (x_cam = H x_world) -> (n, 3) float64"""
        P = np.array([np.asarray(l.p, np.float64).reshape(3) for l in landmarks], np.float64).reshape(-1, 3)
        H = np.asarray(H, np.float64)
        return P @ H[:3, :3].T + H[:3, 3]

    def align_frame(self, K, im_curr, landmarks, H_prev, H_init=None, **params):
        """The pose of im_curr BEFORE anything is tracked: sparse direct image alignment (VoContext.sparse_align) of the pair
        (_im_prev, im_curr) on the landmarks, which are moved into the previous camera's frame on the host (x = H_prev p).  The pair goes
        into the frame store as extend_tracks would put it, so the extend_* calls that follow on the same image push nothing again.
        H_prev: the previous frame's pose (4x4, x_cam = H x_world); H_init: a guess for the new pose (None: H_prev, no motion); params:
        VoContext.align_params' keywords.  -> (H_cur 4x4, info dict: the context's stats plus 'used', the indices of the landmarks of the
        last linearisation).  No level ran (too few landmarks in view): info['status'] != 0 and H_cur is the guess.
        project_landmarks(K, H_cur, landmarks) then gives extend_landmarks(init=) its start positions.  A live lazy session ends here: the
        call takes the plain path, like every call outside the reference's order."""
        from .so3 import rodrigues_mat_to_vec, rodrigues_vec_to_mat
        if self._im_prev is None:
            raise RuntimeError("align_frame needs _im_prev, the frame the landmarks were last seen in")
        self._plain("align_frame", im_curr)
        self._ensure_pair(self._im_prev, im_curr)
        H_prev = np.asarray(H_prev, np.float64)
        X = self._points_in_camera(H_prev, landmarks).astype(np.float32)
        r0 = t0 = None
        if H_init is not None:
            T0 = np.asarray(H_init, np.float64) @ np.linalg.inv(H_prev)
            r0, t0 = rodrigues_mat_to_vec(T0[:3, :3]), T0[:3, 3].copy()
        rv, tv, used, st = self._ctx.sparse_align(K, X, r0, t0, self._ctx.align_params(**params))
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = rodrigues_vec_to_mat(rv), tv
        info = dict(st)
        info["used"] = np.nonzero(used)[0].tolist()
        return T @ H_prev, info

    def project_landmarks(self, K, H, landmarks):
        """the landmarks' pixels under the pose H (4x4, x_cam = H x_world) -> (n, 2) float32; a point at or behind the camera gives NaN,
        which the seeded tracker reads as `start where the keypoint was`"""
        K = np.asarray(K, np.float64).reshape(3, 3)
        Y = self._points_in_camera(H, landmarks)
        with np.errstate(all="ignore"):
            z = np.where(Y[:, 2] > 0, Y[:, 2], np.nan)
            uv = np.stack([K[0, 0] * Y[:, 0] / z + K[0, 2], K[1, 1] * Y[:, 1] / z + K[1, 2]], 1)
        return uv.astype(np.float32)

    # -- the depth filter: candidates that carry a depth and its uncertainty while they wait ---------------------------------------
    def init_seeds(self, candidates, H_ref, depth_mean=None, depth_min=None, landmarks=None, im_ref=None):
        """Depth-filter seeds (VoContext.depth_seeds; the algorithm: tests/depth_model.py) for the candidate keypoints at their newest
        positions in the reference frame im_ref (None: _im_prev, the frame extend_tracks saw last), whose pose is H_ref (4x4,
        x_cam = H x_world).  depth_mean / depth_min: the prior, scene depths; None: the mean and the smallest depth of `landmarks` in
        that camera.  -> DepthSeeds that remember H_ref and the candidates; update_seeds moves them, seed_landmarks reads them."""
        im_ref = self._im_prev if im_ref is None else im_ref
        if im_ref is None:
            raise RuntimeError("init_seeds needs the reference frame: pass im_ref=, or track a frame first")
        if depth_mean is None or depth_min is None:
            if not landmarks:
                raise ValueError("init_seeds needs depth_mean and depth_min, or landmarks to take them from")
            z = self._points_in_camera(H_ref, landmarks)[:, 2]
            z = z[z > 0]
            if not len(z):
                raise ValueError("init_seeds: no landmark in front of the reference camera")
            depth_mean = float(z.mean()) if depth_mean is None else depth_mean
            depth_min = float(z.min()) if depth_min is None else depth_min
        self._plain("init_seeds", im_ref)
        self._ensure_cur(np.ascontiguousarray(im_ref, np.uint8))
        uv = np.array([np.asarray(k.uv, np.float64).reshape(2) for k in candidates], np.float32).reshape(-1, 2)
        s = self._ctx.depth_seeds(uv, depth_mean, depth_min, ref_id=0)
        s.H_ref, s.kps = [np.array(H_ref, np.float64)], list(candidates)
        return s

    def update_seeds(self, K, seeds, H_cur, im_curr=None, **params):
        """One depth-filter update (VoContext.depth_update) of `seeds` against im_curr (None: the frame the store holds) under its pose
        H_cur (4x4, from align_frame, camera_pose or the bundle adjustment); the relative poses H_cur H_ref^-1 are formed in float64 on
        the host.  params: VoContext.depth_params' keywords.  seeds are updated in place -> (result (n,) u8, match_uv (n,2), z (n,),
        stats dict), as VoContext.depth_update"""
        from .so3 import rodrigues_mat_to_vec
        if im_curr is not None:
            self._plain("update_seeds", im_curr)
            self._ensure_cur(np.ascontiguousarray(im_curr, np.uint8))
        H_cur = np.asarray(H_cur, np.float64)
        poses = np.zeros((len(seeds.H_ref), 6))
        for r, H_ref in enumerate(seeds.H_ref):
            T = H_cur @ np.linalg.inv(H_ref)
            poses[r, :3], poses[r, 3:] = np.asarray(rodrigues_mat_to_vec(T[:3, :3])).reshape(3), T[:3, 3]
        seeds.K = np.array(K, np.float64).reshape(3, 3)
        return self._ctx.depth_update(K, poses, seeds, self._ctx.depth_params(**params))

    def seed_landmarks(self, seeds, which="converged", K=None, t_curr=None):
        """The seeds that have converged (which="converged"; "active": every seed not flagged diverged; or a boolean mask) as Landmarks
        in world coordinates, H_ref^-1 (f / mu), with their Keypoints -- shaped like triangulate_tracks' output, so a caller appends them
        where it appends those.  K: None = the intrinsics update_seeds saw last; t_curr: the landmarks' t_latest (None: each
        keypoint's newest frame).  -> (landmarks, their keypoints, the remaining candidates' keypoints).  seeds.depth_sigma holds
        the standard deviation of each seed's distance along its bearing"""
        K = seeds.K if K is None else K
        if K is None:
            raise ValueError("seed_landmarks needs K: no update_seeds call has given one yet")
        K = np.asarray(K, np.float64).reshape(3, 3)
        sd = seeds.seeds
        if isinstance(which, str):
            pick = {"converged": seeds.converged & ~seeds.diverged, "active": ~seeds.diverged}[which]
        else:
            pick = np.asarray(which, bool)
        rows = np.nonzero(pick)[0]
        x, y = (sd["u"][rows].astype(np.float64) - K[0, 2]) / K[0, 0], (sd["v"][rows].astype(np.float64) - K[1, 2]) / K[1, 1]
        f = np.stack([x, y, np.ones(len(rows))], 1) / np.sqrt(x * x + y * y + 1.0)[:, None]
        Xc = f / sd["mu"][rows][:, None]
        P = np.empty((len(rows), 3))
        for r in range(len(seeds.H_ref)):
            m = sd["ref_id"][rows] == r
            Hi = np.linalg.inv(seeds.H_ref[r])
            P[m] = Xc[m] @ Hi[:3, :3].T + Hi[:3, 3]
        kps = [seeds.kps[i] for i in rows]
        lms = [Landmark(k.t_first + k.t_total - 1 if t_curr is None else t_curr, P[i].reshape(3, 1).copy(), k.des) for i, k in enumerate(kps)]
        return lms, kps, [k for i, k in enumerate(seeds.kps) if not pick[i]]

    def bootstrap_check(self, K, list_1, list_2, threshold=1.0, max_h_ratio=0.8, seed=0):
        """Is this frame pair fit for the 2D-2D bootstrap?  One essential_ransac and one find_homography call at the same pixel threshold;
        -> dict e_inliers, h_inliers, h_ratio = h_inliers / max(e_inliers, 1), degenerate = h_ratio > max_h_ratio (COLMAP's
        max_H_inlier_ratio rule): a homography that explains nearly every epipolar inlier means no baseline to speak of or a planar scene,
        and the t of camera_pose(corr='2D-2D') is then not to be trusted.  camera_pose itself is unchanged."""
        if self._ctx is None:
            raise RuntimeError("bootstrap_check needs the device context: track a frame first (or pass ctx=)")
        p1, p2 = self._uv_pairs(list_1, list_2)
        e_st = self._ctx.essential_ransac(np.asarray(K, np.float64), p1, p2, threshold=threshold, prob=0.9999, seed=seed)[4]
        h_st = self._ctx.find_homography(p1, p2, threshold=threshold, seed=seed)[2]
        ratio = h_st["n_inliers"] / max(e_st["n_inliers"], 1)
        return dict(e_inliers=e_st["n_inliers"], h_inliers=h_st["n_inliers"], h_ratio=ratio, degenerate=bool(ratio > max_h_ratio))

    @staticmethod
    def _planar_info(K, Hm, R, t, nrm, st, min_parallax_px):
        """the ranked candidates of VoContext.homography_pose -> (H 4x4 of the best with |t| = 1, or t = 0 for a rotation; info dict)"""
        ns = st["n_solutions"]
        f = (float(K[0][0]) + float(K[1][1])) / 2.0
        # a plane-induced parallax f |t / d| = f (s1 - s3) under min_parallax_px moves no point by more than that: at this pixel scale the
        # homography cannot be told from a rotation, and the direction of its t is noise
        rot = bool(ns == 1 or (st["sigma"][0] - st["sigma"][2]) * f <= min_parallax_px)
        alts = []
        for k in range(ns):
            tn = float(np.linalg.norm(t[k]))
            alts.append(dict(R=R[k].copy(), t=(t[k] / tn if tn > 0 else np.zeros(3)), t_over_d=t[k].copy(), n=nrm[k].copy(),
                             n_good=st["n_good"][k], n_off=st["n_off"][k]))
        H4 = np.eye(4)
        H4[:3, :3] = alts[0]["R"]
        if not rot:
            H4[:3, 3] = alts[0]["t"]
        info = dict(alternatives=alts, n_good=st["n_good"][:ns], n_off=st["n_off"][:ns], n_mask=st["n_mask"], n_solutions=ns,
                    n_distinct=st["n_distinct"], ambiguous=bool(st["ambiguous"]) and not rot, rotation_only=rot, sigma=st["sigma"], homography=Hm)
        return H4, info

    def camera_pose_planar(self, K, list_1, list_2, threshold=3.0, seed=0, normal_hint=None, min_parallax_px=1.0, **kw):
        """Pose from the homography of a planar scene or a pair without a baseline, where camera_pose(corr='2D-2D') has nothing to offer:
        cv2.findHomography(RANSAC, threshold) + cv2.decomposeHomographyMat, ranked by the visibility of the inliers, the Sampson support of the
        points off the plane and the optional plane-normal prior normal_hint (view-1 camera coordinates; a ground plane is (0, 1, 0)).
        -> (inlier indices as a list, H 4x4 view-1 -> view-2 with |t| = 1, info).  info: `alternatives` (every candidate in rank order: R, t
        of unit length, t_over_d, n, n_good, n_off), `ambiguous` (two candidates pass and nothing tells them apart: a plane without
        off-plane points and without a hint -- take the alternatives to the next view), `rotation_only` (the parallax f (s1 - s3) is under
        min_parallax_px: H's t is 0), n_good, n_off, n_mask, n_solutions, n_distinct, sigma, homography.  Further keywords as
        VoContext.homography_pose."""
        if self._ctx is None:
            raise RuntimeError("camera_pose_planar needs the device context: track a frame first (or pass ctx=)")
        Kc = np.asarray(K, np.float64)
        Hm, inliers, hst, R, t, nrm, st = self._ctx.homography_pose(Kc, *self._uv_pairs(list_1, list_2), threshold=threshold, seed=seed,
                                                                   normal_hint=normal_hint, **kw)
        if hst["status"] != 0 or st["status"] != 0:
            raise RuntimeError("findHomography found no model to decompose")
        H4, info = self._planar_info(Kc, Hm, R, t, nrm, st, min_parallax_px)
        return inliers.reshape((-1,)).tolist(), H4, info

    def bootstrap_pose(self, K, list_1, list_2, threshold=1.0, max_h_ratio=0.8, seed=0, normal_hint=None):
        """bootstrap_check's verdict followed by the right model.  -> dict `model`: 'essential' (the pair has structure and a baseline: the
        pose of camera_pose(corr='2D-2D')), 'homography' (planar scene: the best candidate of camera_pose_planar, |t| = 1) or 'rotation' (no
        baseline to speak of: t = 0); `inliers` (a list, of the model used), `H` 4x4 view-1 -> view-2, `ambiguous` (True only for
        'homography': see camera_pose_planar; `info` then holds the alternatives), `check` (bootstrap_check's dict)."""
        if self._ctx is None:
            raise RuntimeError("bootstrap_pose needs the device context: track a frame first (or pass ctx=)")
        Kc = np.asarray(K, np.float64)
        p1, p2 = self._uv_pairs(list_1, list_2)
        _E, Re, te, e_inl, e_st = self._ctx.essential_ransac(Kc, p1, p2, threshold=threshold, prob=0.9999, seed=seed)
        Hm, h_inl, h_st, R, t, nrm, st = self._ctx.homography_pose(Kc, p1, p2, threshold=threshold, seed=seed, pose_threshold=threshold,
                                                                  normal_hint=normal_hint)
        ratio = h_st["n_inliers"] / max(e_st["n_inliers"], 1)
        check = dict(e_inliers=e_st["n_inliers"], h_inliers=h_st["n_inliers"], h_ratio=ratio, degenerate=bool(ratio > max_h_ratio))
        if not check["degenerate"] or h_st["status"] != 0 or st["status"] != 0:
            if e_st["status"] != 0:
                raise RuntimeError("findEssentialMat found no model")
            H4 = np.eye(4)
            H4[:3, :3] = Re
            H4[:3, 3] = te.reshape((3,))
            return dict(model='essential', inliers=e_inl.reshape((-1,)).tolist(), H=H4, ambiguous=False, check=check, info=None)
        H4, info = self._planar_info(Kc, Hm, R, t, nrm, st, threshold)
        return dict(model='rotation' if info["rotation_only"] else 'homography', inliers=h_inl.reshape((-1,)).tolist(), H=H4,
                    ambiguous=info["ambiguous"], check=check, info=info)
