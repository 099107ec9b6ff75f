"""Array-native front end: numpy in, numpy out, one VoContext per (host thread, GPU).

Thin wrapper over the C ABI (include/vo_mi355x.h).  The drop-in classes in
extractor.py / bundle_adjuster.py are built on top of this.

Batched contexts: `VoContext(..., batch=B)` carries B independent sequences of identical shape in lockstep (one
launch serves all of them).  With B > 1 every array argument / result gains a leading dimension of length B; with
B == 1 (default) the arrays are exactly those of the single-sequence API.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import AlignParams, AlignStats, BaParams, BaStats, BriefParams, DepthParams, DepthSeed, DepthStats, EssParams, EssStats, FundParams, FundStats, GMatchParams, HomParams, HomStats, HposeParams, HposeStats, KltParams, OrbKp, OrbParams, SiftKp, PnpParams, PnpStats, Sim3Params, Sim3Stats, StParams, SubpixParams, Tuning, VoError, as_c, ptr

# vo_set_klt_predict modes (include/vo_mi355x.h)
KLT_PREDICT_MODES = {"off": 0, "constant_velocity": 1}


class DepthSeeds:
    """What VoContext.depth_seeds returns and depth_update updates: seeds, a structured array of vo_depth_seed rows (mu, sigma2, a, b,
    z_range, u, v, ref_id, flags); patches (.., 100) u8, the 10 x 10 reference patches; ok (..,) bool, False where no patch could be cut.
    Extractor.init_seeds adds H_ref, the list of 4x4 reference poses ref_id indexes, and kps, the candidate keypoints; update_seeds K"""

    def __init__(self, seeds, patches, ok, H_ref=None, kps=None, K=None):
        self.seeds, self.patches, self.ok, self.H_ref, self.kps, self.K = seeds, patches, ok, H_ref, kps, K

    def __len__(self):
        return self.seeds.shape[-1]

    @property
    def converged(self):
        return (self.seeds["flags"] & _lib.DEPTH_CONVERGED) != 0

    @property
    def diverged(self):
        return (self.seeds["flags"] & _lib.DEPTH_DIVERGED) != 0

    @property
    def observations(self):
        return self.seeds["flags"] >> _lib.DEPTH_OBS_SHIFT

    @property
    def depth_sigma(self):
        """the standard deviation of each seed's distance along its bearing: sqrt(sigma2) / mu^2"""
        return np.sqrt(self.seeds["sigma2"]) / self.seeds["mu"] ** 2


class VoContext:
    # vo_tuning fields applied to every NEW context (a test module forces one kernel family for all the contexts its tests make this way; the
    # library itself reads no tuning from the environment)
    default_tuning = {}

    def __init__(self, width, height, max_pts=4096, device=0, max_level=3, win=31, batch=1):
        self._L = _lib.load()
        self._h = C.c_void_p()
        rc = self._L.vo_ctx_create_batched(device, width, height, max_pts, max_level, win, batch, C.byref(self._h))
        if rc != 0:
            msg = self._L.vo_last_error(None)
            raise VoError(rc, msg.decode() if msg else "vo_ctx_create failed")
        self.width, self.height, self.max_pts = width, height, max_pts
        self.max_level, self.win, self.device, self.batch = max_level, win, device, batch
        self._st_max_corners = 1000
        self._corner_slots = 1000       # corner slots the last detection could fill (subpix_read, brief_read)
        self._klt_levels = max_level + 1
        self.comm_ranks, self.comm_rank = 1, 0
        if self.default_tuning:
            self.set_tuning(**self.default_tuning)

    # -- lifetime -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.vo_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc):
        if rc != 0:
            msg = self._L.vo_last_error(self._h)
            raise VoError(rc, msg.decode() if msg else "")

    def sync(self):
        self._ck(self._L.vo_sync(self._h))

    def tuning(self):
        """-> dict of the vo_tuning fields in effect (0 = the library's rule)"""
        t = Tuning()
        self._ck(self._L.vo_get_tuning(self._h, C.byref(t)))
        return {k: getattr(t, k) for k in _lib.TUNING_FIELDS}

    def set_tuning(self, **fields):
        """force forms the library otherwise chooses by rule (include/vo_mi355x.h: vo_tuning; parity tests and A/B measurements).  Fields not
        named keep their value; `set_tuning(**dict.fromkeys(ctx.tuning(), 0))` restores the rules."""
        t = Tuning()
        self._ck(self._L.vo_get_tuning(self._h, C.byref(t)))
        for k, v in fields.items():
            if k not in _lib.TUNING_FIELDS:
                raise ValueError("set_tuning: unknown field %r" % k)
            setattr(t, k, int(v))
        self._ck(self._L.vo_set_tuning(self._h, C.byref(t)))

    # -- batch helpers --------------------------------------------------------------------------
    def _in(self, a, dtype, per_seq_shape):
        """-> C-contiguous [batch, *per_seq_shape] view of the caller's array (batch dim optional when batch == 1)"""
        a = np.asarray(a, dtype=dtype)
        want = (self.batch,) + tuple(per_seq_shape)
        if a.shape != want:
            if self.batch == 1:
                a = a.reshape(want)
            else:
                raise ValueError("expected array of shape %r, got %r" % (want, a.shape))
        return np.ascontiguousarray(a)

    def _out(self, a):
        return a[0] if self.batch == 1 else a

    # -- frames ---------------------------------------------------------------------------------
    def set_prefilter(self, d=5, sigma_color=1.5, sigma_space=1.5):
        """cv2.bilateralFilter(img, d, sigmaColor, sigmaSpace) on every frame entering the frame store (the reference
        loader's pre-filter, loader.py:16-20,86); d = 0 switches it off."""
        self._ck(self._L.vo_set_prefilter(self._h, int(d), float(sigma_color), float(sigma_space)))

    def bilateral(self, img, d=5, sigma_color=1.5, sigma_space=1.5):
        """cv2.bilateralFilter(img, d, sigmaColor, sigmaSpace) -> filtered uint8 image (Loader.getImage, reference
        loader.py:86).  Runs the fused pre-filter of the frame store and reads level 0 back, i.e. it PUSHES a frame: use a
        context of its own (vo_mi355x.Loader does), not the one an Extractor is tracking with."""
        self.set_prefilter(d, sigma_color, sigma_space)
        try:
            self.push_frame(img)
            return self.pyramid_read(1, 0)[0]
        finally:
            self.set_prefilter(0)

    @staticmethod
    def _k4(K, name):
        """a 3 x 3 camera matrix or (fx, fy, cx, cy) -> float64 [4]"""
        K = np.asarray(K, np.float64)
        if K.shape == (3, 3):
            return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
        if K.shape != (4,):
            raise ValueError("%s: a 3 x 3 matrix or (fx, fy, cx, cy), got shape %r" % (name, K.shape))
        return np.ascontiguousarray(K)

    def set_undistort(self, K, dist, new_K=None):
        """cv2.undistort(img, K, dist, None, new_K) on every frame entering the frame store, in front of the bilateral pre-filter
        (vo_set_undistort).  K, new_K: 3 x 3 or (fx, fy, cx, cy), new_K = None: K; dist: (k1, k2, p1, p2[, k3[, k4, k5, k6]]) or empty."""
        K4 = self._k4(K, "K")
        N4 = None if new_K is None else self._k4(new_K, "new_K")
        d = np.ascontiguousarray(np.asarray([] if dist is None else dist, np.float64).reshape(-1))
        self._ck(self._L.vo_set_undistort(self._h, ptr(K4, C.c_double), ptr(d, C.c_double) if d.size else None, int(d.size),
                                          None if N4 is None else ptr(N4, C.c_double)))

    def clear_undistort(self):
        self._ck(self._L.vo_clear_undistort(self._h))

    def get_undistort(self):
        """-> None when off, else dict(K=(fx, fy, cx, cy), dist=[8], new_K=(fx', fy', cx', cy')) as float64 arrays"""
        on = C.c_int32()
        K, d, N = np.zeros(4), np.zeros(8), np.zeros(4)
        self._ck(self._L.vo_get_undistort(self._h, C.byref(on), ptr(K, C.c_double), ptr(d, C.c_double), ptr(N, C.c_double)))
        return dict(K=K, dist=d, new_K=N) if on.value else None

    def _ingest_call(self, name, fn, img):
        """the body of undistort() / clahe(): `img` ([h, w] uint8, [batch, h, w] on a batched context) through the stage `fn` alone into a
        fresh array.  A view whose rows are `stride` >= w bytes apart (buf[..., :w] of a C-contiguous buffer) is read in place."""
        img = np.asarray(img)
        if img.dtype != np.uint8:
            raise ValueError("%s: expected uint8" % name)
        h, w = self.height, self.width
        stride = img.strides[-2] if img.ndim >= 2 else 0
        rows_in_place = (img.shape == (self.batch, h, w) and img.strides == (h * stride, stride, 1)) or \
                        (self.batch == 1 and img.shape == (h, w) and img.strides == (stride, 1))
        if not (rows_in_place and stride >= w):
            img, stride = self._in(img, np.uint8, (h, w)), w
        out = np.empty((self.batch, h, w), np.uint8)
        self._ck(fn(self._h, ptr(img, C.c_uint8), stride, ptr(out, C.c_uint8)))
        return self._out(out)

    def undistort(self, img):
        """cv2.undistort of `img` with the setting of set_undistort (vo_undistort, see _ingest_call); the frame store is not touched"""
        return self._ingest_call("undistort", self._L.vo_undistort, img)

    def undistort_map_read(self):
        """the fixed-point map of the setting (vo_undistort_map_read): dict of sxy (h, w, 2) i16 = the top-left tap (sx, sy),
        frac (h, w) u16 = fy5 * 32 + fx5, outside (h, w) u8"""
        sxy = np.empty((self.height, self.width, 2), np.int16)
        frac = np.empty((self.height, self.width), np.uint16)
        out = np.empty((self.height, self.width), np.uint8)
        self._ck(self._L.vo_undistort_map_read(self._h, ptr(sxy, C.c_int16), ptr(frac, C.c_uint16), ptr(out, C.c_uint8)))
        return dict(sxy=sxy, frac=frac, outside=out)

    @staticmethod
    def _undistort_args(undistort):
        """dict(K=, dist=[, new_K=]) -- cv2.undistort's arguments -> (K, dist, new_K)"""
        unknown = set(undistort) - {"K", "dist", "new_K"}
        if unknown or "K" not in undistort:
            raise ValueError("undistort: a dict with K, dist and optionally new_K, got keys %r" % sorted(undistort))
        return undistort["K"], undistort.get("dist"), undistort.get("new_K")

    @staticmethod
    def _clahe_args(clahe):
        """(clip_limit, (tiles_x, tiles_y)) -- cv2.createCLAHE's arguments -- or a dict with clip_limit / tiles -> (float, int, int)"""
        if isinstance(clahe, dict):
            unknown = set(clahe) - {"clip_limit", "tiles"}
            if unknown:
                raise ValueError("clahe: a dict with clip_limit and tiles, got keys %r" % sorted(clahe))
            clahe = (clahe.get("clip_limit", 40.0), clahe.get("tiles", (8, 8)))
        try:
            clip, (tx, ty) = clahe
            clip, tx, ty = float(clip), int(tx), int(ty)
        except (TypeError, ValueError):
            raise ValueError("clahe: (clip_limit, (tiles_x, tiles_y)), got %r" % (clahe,))
        return clip, tx, ty

    def set_clahe(self, clip_limit=40.0, tiles=(8, 8)):
        """cv2.createCLAHE(clip_limit, tiles).apply(img) on every frame entering the frame store, behind the undistortion and in front of the
        bilateral pre-filter (vo_set_clahe).  tiles = (tiles_x, tiles_y), 1 .. 16 each; clip_limit = 0: no clipping."""
        clip, tx, ty = self._clahe_args((clip_limit, tiles))
        self._ck(self._L.vo_set_clahe(self._h, clip, tx, ty))

    def clear_clahe(self):
        self._ck(self._L.vo_clear_clahe(self._h))

    def apply_ingest(self, undistort, clahe, clear_missing):
        """undistort = dict(K=, dist=[, new_K=]), clahe = (clip_limit, (tiles_x, tiles_y)) or a dict, both validated before either is set.
        None: with clear_missing a setting the context has is switched off, without it no call at all (the context keeps what it has)."""
        u = None if undistort is None else self._undistort_args(undistort)
        cl = None if clahe is None else self._clahe_args(clahe)
        if u is not None:
            self.set_undistort(*u)
        elif clear_missing and self.get_undistort() is not None:
            self.clear_undistort()
        if cl is not None:
            self.set_clahe(cl[0], cl[1:])
        elif clear_missing and self.get_clahe() is not None:
            self.clear_clahe()

    def get_clahe(self):
        """-> None when off, else (clip_limit, (tiles_x, tiles_y))"""
        on, tx, ty, clip = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
        self._ck(self._L.vo_get_clahe(self._h, C.byref(on), C.byref(clip), C.byref(tx), C.byref(ty)))
        return (clip.value, (tx.value, ty.value)) if on.value else None

    def clahe(self, img):
        """CLAHE of `img` with the setting of set_clahe (vo_clahe, see _ingest_call): CLAHE alone, not the undistortion in front of it; the
        frame store is not touched"""
        return self._ingest_call("clahe", self._L.vo_clahe, img)

    def clahe_lut_read(self):
        """the tables the last launch wrote (vo_clahe_lut_read): uint8 [tiles_y, tiles_x, 256] ([batch, ...] on a batched context)"""
        g = self.get_clahe()
        if g is None:
            self._ck(self._L.vo_clahe_lut_read(self._h, None))               # the library's own refusal
        tx, ty = g[1]
        lut = np.empty((self.batch, ty, tx, 256), np.uint8)
        self._ck(self._L.vo_clahe_lut_read(self._h, ptr(lut, C.c_uint8)))
        return self._out(lut)

    def push_frame(self, img):
        img = np.asarray(img)
        if img.dtype != np.uint8:
            raise ValueError("push_frame: expected uint8")
        img = self._in(img, np.uint8, (self.height, self.width))
        self._ck(self._L.vo_frame_push(self._h, ptr(img, C.c_uint8), self.width))

    def upload_sequence(self, frames):
        """frames: [n_frames, h, w] (batch == 1) or [batch, n_frames, h, w]"""
        frames = np.asarray(frames, np.uint8)
        if frames.ndim == 3 and self.batch == 1:
            frames = frames[None]
        assert frames.ndim == 4 and frames.shape[0] == self.batch and frames.shape[2:] == (self.height, self.width)
        frames = np.ascontiguousarray(frames)
        self._ck(self._L.vo_seq_upload(self._h, ptr(frames, C.c_uint8), frames.shape[1]))

    def push_frame_resident(self, idx):
        self._ck(self._L.vo_frame_push_resident(self._h, int(idx)))

    def level_size(self, level):
        w, h = C.c_int32(), C.c_int32()
        self._ck(self._L.vo_pyramid_level_size(self._h, level, C.byref(w), C.byref(h)))
        return w.value, h.value

    def pyramid_read(self, which, level, seq=0):
        """-> (img uint8 [h,w], deriv int16 [h,w,2]) of the prev (which=0) / cur (which=1) frame of sequence `seq`."""
        w, h = self.level_size(level)
        img = np.empty((h, w), np.uint8)
        der = np.empty((h, w, 2), np.int16)
        self._ck(self._L.vo_pyramid_read_seq(self._h, seq, which, level, ptr(img, C.c_uint8), ptr(der, C.c_int16)))
        return img, der

    # -- KLT ------------------------------------------------------------------------------------
    def klt_params(self, win=None, max_level=None, max_count=30, epsilon=0.03, min_eig_threshold=1e-4):
        p = KltParams()
        self._L.vo_klt_default_params(C.byref(p))
        p.win = self.win if win is None else win
        p.max_level = self.max_level if max_level is None else max_level
        p.max_count, p.epsilon, p.min_eig_threshold = max_count, epsilon, min_eig_threshold
        return p

    def _npts(self, p):
        p = np.asarray(p, np.float32)
        if self.batch == 1:
            p = p.reshape(1, -1, 2)
        if p.ndim != 3 or p.shape[0] != self.batch or p.shape[2] != 2:
            raise ValueError("points must have shape [batch, n, 2]")
        return np.ascontiguousarray(p), p.shape[1]

    def _guess(self, init, n):
        """init of klt_track / klt_track_fb -> (the guess array or None, its pointer or NULL)"""
        if init is None:
            return None, None
        g, ng = self._npts(init)
        if ng != n:
            raise ValueError("init must have the shape of p0")
        return g, ptr(g, C.c_float)

    def klt_track(self, p0, params=None, return_iters=False, init=None):
        """prev -> cur tracking.  p0 (n,2) float32 -> p1 (n,2) f32, status (n,) u8, err (n,) f32  [leading batch dim if batch > 1]
        init (the shape of p0, or None): a start position per point for the top pyramid level, OpenCV's OPTFLOW_USE_INITIAL_FLOW
        (vo_klt_track_init); a guess with a non-finite component starts from p0, init = p0 gives the bits of init = None."""
        p0, n = self._npts(p0)
        B = self.batch
        prm = params if params is not None else self.klt_params()
        p1 = np.zeros((B, n, 2), np.float32)
        st = np.zeros((B, n), np.uint8)
        err = np.zeros((B, n), np.float32)
        it = np.full((B, n, prm.max_level + 1), -1, np.int32)
        g, gp = self._guess(init, n)
        if g is None:
            self._ck(self._L.vo_klt_track(self._h, ptr(p0, C.c_float), n, C.byref(prm), ptr(p1, C.c_float),
                                          ptr(st, C.c_uint8), ptr(err, C.c_float), ptr(it, C.c_int32)))
        else:
            self._ck(self._L.vo_klt_track_init(self._h, ptr(p0, C.c_float), gp, n, C.byref(prm), ptr(p1, C.c_float),
                                               ptr(st, C.c_uint8), ptr(err, C.c_float), ptr(it, C.c_int32)))
        if return_iters:
            return self._out(p1), self._out(st), self._out(err), self._out(it)
        return self._out(p1), self._out(st), self._out(err)

    def klt_track_fb(self, p0, params=None, return_iters=False, init=None):
        """klt_track with the forward-backward check in the same launch (vo_klt_track_fb): p1, status, err exactly as klt_track, plus
        p0r (n,2) f32 = the backward track of p1 (current -> previous frame) and fb_err (n,) f32 = max(|p0 - p0r|) over x, y.  The ok flags
        (fb_err < the context's threshold) come from fb_read(n).  init: as in klt_track, for the forward pass (vo_klt_track_fb_init); the
        backward pass starts at p1 as always."""
        p0, n = self._npts(p0)
        B = self.batch
        prm = params if params is not None else self.klt_params()
        p1 = np.zeros((B, n, 2), np.float32)
        st = np.zeros((B, n), np.uint8)
        err = np.zeros((B, n), np.float32)
        p0r = np.zeros((B, n, 2), np.float32)
        fb_err = np.zeros((B, n), np.float32)
        it = np.full((B, n, prm.max_level + 1), -1, np.int32)
        g, gp = self._guess(init, n)
        if g is None:
            self._ck(self._L.vo_klt_track_fb(self._h, ptr(p0, C.c_float), n, C.byref(prm), ptr(p1, C.c_float), ptr(st, C.c_uint8),
                                             ptr(err, C.c_float), ptr(p0r, C.c_float), ptr(fb_err, C.c_float), ptr(it, C.c_int32)))
        else:
            self._ck(self._L.vo_klt_track_fb_init(self._h, ptr(p0, C.c_float), gp, n, C.byref(prm), ptr(p1, C.c_float), ptr(st, C.c_uint8),
                                                  ptr(err, C.c_float), ptr(p0r, C.c_float), ptr(fb_err, C.c_float), ptr(it, C.c_int32)))
        out = (self._out(p1), self._out(st), self._out(err), self._out(p0r), self._out(fb_err))
        return out + (self._out(it),) if return_iters else out

    def set_fb_check(self, max_err=np.inf):
        """threshold of the forward-backward check (vo_set_fb_check): a finite value makes tracks_track and the closed loop's TRACK stage
        drop every point with fb_err >= max_err (or NaN); np.inf (the default) turns it off.  Rounded to float32 once."""
        self._ck(self._L.vo_set_fb_check(self._h, C.c_float(float(max_err))))

    def get_fb_check(self):
        v = C.c_float(0.0)
        self._ck(self._L.vo_get_fb_check(self._h, C.byref(v)))
        return v.value

    def fb_read(self, n):
        """(ok (n,) bool, fb_err (n,) f32) of the last track's dense point set, if it ran with the check [leading batch dim if batch > 1]"""
        B = self.batch
        ok = np.zeros((B, n), np.uint8)
        fb_err = np.zeros((B, n), np.float32)
        self._ck(self._L.vo_fb_read(self._h, ptr(ok, C.c_uint8), ptr(fb_err, C.c_float), n))
        return self._out(ok.astype(bool)), self._out(fb_err)

    def set_klt_predict(self, mode="off"):
        """motion-predicted start of the tracker (vo_set_klt_predict): "constant_velocity" (or 1) makes tracks_track and the closed loop's
        TRACK stage start every point at uv + (uv - prev) from the track's own history (uv without one); "off" (or 0, the default): at uv."""
        self._ck(self._L.vo_set_klt_predict(self._h, int(KLT_PREDICT_MODES.get(mode, mode))))

    def get_klt_predict(self):
        """the mode as its name ("off" / "constant_velocity")"""
        v = C.c_int32(-1)
        self._ck(self._L.vo_get_klt_predict(self._h, C.byref(v)))
        return {code: name for name, code in KLT_PREDICT_MODES.items()}[v.value]

    def klt_guess_read(self, n):
        """(n,2) f32: the start positions the last track's predictor wrote, in the tracker's point order; dead slots NaN
        [leading batch dim if batch > 1]"""
        g = np.zeros((self.batch, n, 2), np.float32)
        self._ck(self._L.vo_klt_guess_read(self._h, ptr(g, C.c_float), n))
        return self._out(g)

    # -- sub-pixel corner refinement ---------------------------------------------------------------
    def subpix_params(self, win=(5, 5), zero_zone=(-1, -1), max_count=40, epsilon=0.001):
        """cv2.cornerSubPix's arguments: win / zero_zone are (x, y) half sizes (win 1..7, zero_zone -1 = none), criteria = (max_count, epsilon)"""
        p = SubpixParams()
        self._L.vo_subpix_default_params(C.byref(p))
        p.win_x, p.win_y = int(win[0]), int(win[1])
        p.zero_x, p.zero_y = int(zero_zone[0]), int(zero_zone[1])
        p.max_count, p.epsilon = int(max_count), float(epsilon)
        return p

    @staticmethod
    def _which(which):
        """the frame a corner stage works on: "prev" / "cur" or the library's 0 / 1"""
        return int({"prev": 0, "cur": 1}.get(which, which))

    def _cut_corner_rows(self, n, dead, **cols):
        """per sequence the rows in front of the first slot the detection did not fill (dead [B, n]) -> dict of copies [list of B dicts if batch > 1]"""
        ms = [int(np.argmax(d)) if d.any() else n for d in dead]
        out = [{k: v[b, :m].copy() for k, v in cols.items()} for b, m in enumerate(ms)]
        return out[0] if self.batch == 1 else out

    def corner_subpix(self, corners, which="cur", params=None, return_info=False):
        """cv2.cornerSubPix on a frame of the frame store (vo_corner_subpix): corners (n,2) f32 -> refined (n,2) f32, with return_info also
        iters (n,) i32 and flags (n,) u8 (0 stopped, 1 singular, 2 left the image, 3 reverted, 4 input not usable)  [leading batch dim if
        batch > 1].  which: "cur" (1) or "prev" (0).  Rows that are not finite or outside the image come back unchanged."""
        p, n = self._npts(corners)
        B = self.batch
        prm = params if params is not None else self.subpix_params()
        out = p.copy()
        it = np.zeros((B, n), np.int32)
        fl = np.zeros((B, n), np.uint8)
        self._ck(self._L.vo_corner_subpix(self._h, self._which(which), ptr(p, C.c_float), n, C.byref(prm), ptr(out, C.c_float), ptr(it, C.c_int32),
                                          ptr(fl, C.c_uint8)))
        if return_info:
            return self._out(out), self._out(it), self._out(fl)
        return self._out(out)

    def set_subpix(self, params=None):
        """refine the corners of tracks_detect and of the closed loop's DETECT stage before they become tracks (vo_set_subpix): a
        subpix_params() struct, a dict of its keywords, or None = off (the default)"""
        if isinstance(params, dict):
            params = self.subpix_params(**params)
        self._ck(self._L.vo_set_subpix(self._h, None if params is None else C.byref(params)))

    def get_subpix(self):
        """None when off, else the SubpixParams in effect"""
        on, p = C.c_int32(0), SubpixParams()
        self._ck(self._L.vo_get_subpix(self._h, C.byref(on), C.byref(p)))
        return p if on.value else None

    def subpix_read(self, n=None):
        """what the last refined detection started from (vo_subpix_read): dict of raw (m,2) f32 = the integer corners, iters (m,) i32,
        flags (m,) u8 per sequence [list of B dicts if batch > 1]; the refined positions are in the tracks.  n: corner slots to read
        (default: all the detection could fill); slots the detection did not fill hold NaN and are cut off."""
        B = self.batch
        if n is None:
            n = self._corner_slots
        raw = np.zeros((B, n, 2), np.float32)
        it = np.zeros((B, n), np.int32)
        fl = np.zeros((B, n), np.uint8)
        self._ck(self._L.vo_subpix_read(self._h, ptr(raw, C.c_float), ptr(it, C.c_int32), ptr(fl, C.c_uint8), n))
        return self._cut_corner_rows(n, np.isnan(raw).any(axis=2), raw=raw, iters=it, flags=fl)

    # -- oriented BRIEF descriptor -------------------------------------------------------------------
    @staticmethod
    def brief_default_pattern():
        """(256, 4) int8: rows (x1, y1, x2, y2) of the default sampling table (vo_brief_default_pattern; needs no context)"""
        out = np.zeros((256, 4), np.int8)
        rc = _lib.load().vo_brief_default_pattern(ptr(out, C.c_int8))
        if rc != 0:
            raise VoError(rc, "vo_brief_default_pattern")
        return out

    def brief_params(self, n_bits=256):
        p = BriefParams()
        self._L.vo_brief_default_params(C.byref(p))
        p.n_bits = int(n_bits)
        return p

    @staticmethod
    def _brief_pattern(pattern):
        """None (the default table) or 256 rows (x1, y1, x2, y2) -> a contiguous int8 array or None; the library checks the values"""
        if pattern is None:
            return None
        p = np.asarray(pattern)
        if p.size != 1024:
            raise ValueError("a BRIEF pattern has 256 rows (x1, y1, x2, y2)")
        if (p != np.clip(p, -128, 127)).any() or (p != np.rint(p)).any():
            raise ValueError("BRIEF pattern coordinates are int8")
        return np.ascontiguousarray(p.reshape(256, 4), np.int8)

    def brief_compute(self, corners, which="cur", params=None, pattern=None):
        """oriented BRIEF at corners (n,2) f32 on a frame of the frame store (vo_brief_compute) -> desc (n,32) u8, angle (n,) f32 degrees,
        flags (n,) u8 (0 described, 1 within 24 pixels of a border, 2 not finite)  [leading batch dim if batch > 1].  which: "cur" (1) or
        "prev" (0); pattern: 256 rows (x1, y1, x2, y2) in [-15, 15], None = the default table."""
        p, n = self._npts(corners)
        B = self.batch
        prm = params if params is not None else self.brief_params()
        pat = self._brief_pattern(pattern)
        desc = np.zeros((B, n, 32), np.uint8)
        ang = np.zeros((B, n), np.float32)
        fl = np.zeros((B, n), np.uint8)
        self._ck(self._L.vo_brief_compute(self._h, self._which(which), ptr(p, C.c_float), n, C.byref(prm), ptr(pat, C.c_int8), ptr(desc, C.c_uint8),
                                          ptr(ang, C.c_float), ptr(fl, C.c_uint8)))
        return self._out(desc), self._out(ang), self._out(fl)

    def set_brief(self, params=None, pattern=None):
        """describe the corners of tracks_detect and of the closed loop's DETECT stage (vo_set_brief): True or a brief_params() struct = on,
        None / False = off (the default); pattern as in brief_compute.  The descriptors go to a side buffer (brief_read)."""
        if params is None or params is False:
            self._ck(self._L.vo_set_brief(self._h, None, None))
            return
        if params is True:
            params = self.brief_params()
        self._ck(self._L.vo_set_brief(self._h, C.byref(params), ptr(self._brief_pattern(pattern), C.c_int8)))

    def get_brief(self):
        """None when off, else the BriefParams in effect"""
        on, p = C.c_int32(0), BriefParams()
        self._ck(self._L.vo_get_brief(self._h, C.byref(on), C.byref(p)))
        return p if on.value else None

    def brief_pattern_read(self):
        """(256, 4) int8: the sampling table in effect (the default one when off)"""
        out = np.zeros((256, 4), np.int8)
        self._ck(self._L.vo_brief_pattern_read(self._h, ptr(out, C.c_int8)))
        return out

    def brief_read(self, n=None):
        """the descriptors of the last detection that described (vo_brief_read), in corner order: dict of desc (m,32) u8, angle (m,) f32,
        flags (m,) u8 per sequence [list of B dicts if batch > 1].  n: corner slots to read (default: all the detection could fill); slots
        the detection did not fill carry flags = 2 and are cut off."""
        B = self.batch
        if n is None:
            n = self._corner_slots
        desc = np.zeros((B, n, 32), np.uint8)
        ang = np.zeros((B, n), np.float32)
        fl = np.zeros((B, n), np.uint8)
        self._ck(self._L.vo_brief_read(self._h, ptr(desc, C.c_uint8), ptr(ang, C.c_float), ptr(fl, C.c_uint8), n))
        return self._cut_corner_rows(n, fl == 2, desc=desc, angle=ang, flags=fl)

    def points_upload(self, p):
        p, n = self._npts(p)
        self._ck(self._L.vo_points_upload(self._h, ptr(p, C.c_float), n))

    def points_download(self, n, return_iters=False):
        B = self.batch
        p = np.zeros((B, n, 2), np.float32)
        st = np.zeros((B, n), np.uint8)
        err = np.zeros((B, n), np.float32)
        it = np.full((B, n, self._klt_levels), -1, np.int32) if return_iters else None
        self._ck(self._L.vo_points_download(self._h, ptr(p, C.c_float), ptr(st, C.c_uint8), ptr(err, C.c_float),
                                            ptr(it, C.c_int32), n))
        if return_iters:
            return self._out(p), self._out(st), self._out(err), self._out(it)
        return self._out(p), self._out(st), self._out(err)

    def klt_track_resident(self, n, params=None):
        prm = params if params is not None else self.klt_params()
        self._klt_levels = prm.max_level + 1
        self._ck(self._L.vo_klt_track_resident(self._h, n, C.byref(prm)))

    # -- Shi-Tomasi -----------------------------------------------------------------------------
    def st_params(self, max_corners=1000, quality_level=0.03, min_distance=7, block_size=31, use_harris=False, harris_k=0.04, fast_threshold=0):
        """fast_threshold: 0 (default) = the Shi-Tomasi / Harris response; 1..254 = the FAST-9/16 corner score at that threshold
        (cv2.FastFeatureDetector's `response`) is ranked instead, everything behind the response map unchanged"""
        p = StParams()
        self._L.vo_st_default_params(C.byref(p))
        p.max_corners, p.quality_level, p.min_distance, p.block_size = max_corners, quality_level, min_distance, block_size
        p.use_harris, p.harris_k = (1 if use_harris else 0), float(harris_k)
        p.fast_threshold = int(fast_threshold)
        return p

    def _corners(self, out, n_out):
        res = [out[b, :n_out[b]].copy() for b in range(self.batch)]
        return res[0] if self.batch == 1 else res

    def shi_tomasi(self, cur_pts=None, mask_radius=7, mask=None, params=None):
        """Re-detection on the CURRENT frame -> corners (m,2) float32 (integer-valued x,y) [list of B arrays if batch > 1]"""
        prm = params if params is not None else self.st_params()
        n_cur, pp = 0, None
        if cur_pts is not None and np.size(cur_pts):
            cur_pts, n_cur = self._npts(cur_pts)
            pp = ptr(cur_pts, C.c_float)
        mp = None
        if mask is not None:
            mask = self._in(mask, np.uint8, (self.height, self.width))
            mp = ptr(mask, C.c_uint8)
        mc = prm.max_corners if prm.max_corners > 0 else 4096
        out = np.zeros((self.batch, mc, 2), np.float32)
        n_out = np.zeros(self.batch, np.int32)
        self._ck(self._L.vo_shi_tomasi(self._h, pp, n_cur, int(mask_radius), mp, C.byref(prm), ptr(out, C.c_float),
                                       ptr(n_out, C.c_int32)))
        return self._corners(out, n_out)

    def shi_tomasi_resident(self, n_cur, mask_radius=7, params=None, limit=None):
        """limit: None, or a corner limit per sequence (an int for all of them, or [batch] ints): sequence b keeps the first
        min(max(limit[b], 0), max_corners) corners of the unlimited call (vo_shi_tomasi_resident_limit, the closed loop's detection)"""
        prm = params if params is not None else self.st_params()
        if limit is None:
            self._ck(self._L.vo_shi_tomasi_resident(self._h, n_cur, int(mask_radius), C.byref(prm)))
        else:
            lim = np.ascontiguousarray(np.broadcast_to(np.asarray(limit, np.int32).reshape(-1), (self.batch,)))
            self._ck(self._L.vo_shi_tomasi_resident_limit(self._h, n_cur, int(mask_radius), C.byref(prm), ptr(lim, C.c_int32)))
        self._st_max_corners = prm.max_corners

    def shi_tomasi_fetch(self):
        mc = self._st_max_corners if self._st_max_corners > 0 else 4096
        out = np.zeros((self.batch, mc, 2), np.float32)
        n_out = np.zeros(self.batch, np.int32)
        self._ck(self._L.vo_shi_tomasi_fetch(self._h, ptr(out, C.c_float), ptr(n_out, C.c_int32)))
        return self._corners(out, n_out)

    def shi_tomasi_read(self):
        eig = np.empty((self.batch, self.height, self.width), np.float32)
        mask = np.empty((self.batch, self.height, self.width), np.uint8)
        nc = np.zeros(self.batch, np.int32)
        self._ck(self._L.vo_shi_tomasi_read(self._h, ptr(eig, C.c_float), ptr(mask, C.c_uint8), ptr(nc, C.c_int32)))
        if self.batch == 1:
            return eig[0], mask[0], int(nc[0])
        return eig, mask, nc

    # -- DLT ------------------------------------------------------------------------------------
    def _dlt_inputs(self, P0, P1, uv0, uv1, K, H0, H1):
        P0, P1 = self._in(P0, np.float32, (3, 4)), self._in(P1, np.float32, (3, 4))
        uv0, n = self._npts(uv0)
        uv1, n1 = self._npts(uv1)
        assert n == n1
        if K is not None:
            K, H0, H1 = self._in(K, np.float64, (3, 3)), self._in(H0, np.float64, (4, 4)), self._in(H1, np.float64, (4, 4))
        return P0, P1, uv0, uv1, n, K, H0, H1

    def triangulate(self, P0, P1, uv0, uv1, K=None, H0=None, H1=None):
        """cv2.triangulatePoints replacement.  -> X4 (4,n) f32 [, depth1 (n,) f64, reproj (n,) f64]"""
        P0, P1, uv0, uv1, n, K, H0, H1 = self._dlt_inputs(P0, P1, uv0, uv1, K, H0, H1)
        B, d = self.batch, C.c_double
        X4 = np.zeros((B, 4, n), np.float32)
        if K is None:
            self._ck(self._L.vo_triangulate_dlt(self._h, ptr(P0, C.c_float), ptr(P1, C.c_float), ptr(uv0, C.c_float),
                                                ptr(uv1, C.c_float), n, ptr(X4, C.c_float), None, None, None, None, None))
            return self._out(X4)
        depth, reproj = np.zeros((B, n)), np.zeros((B, n))
        self._ck(self._L.vo_triangulate_dlt(self._h, ptr(P0, C.c_float), ptr(P1, C.c_float), ptr(uv0, C.c_float),
                                            ptr(uv1, C.c_float), n, ptr(X4, C.c_float), ptr(K, d), ptr(H0, d), ptr(H1, d),
                                            ptr(depth, d), ptr(reproj, d)))
        return self._out(X4), self._out(depth), self._out(reproj)

    def dlt_upload(self, P0, P1, uv0, uv1, K=None, H0=None, H1=None):
        P0, P1, uv0, uv1, n, K, H0, H1 = self._dlt_inputs(P0, P1, uv0, uv1, K, H0, H1)
        self._dlt_n, self._dlt_stats = n, K is not None
        d = C.c_double
        self._ck(self._L.vo_dlt_upload(self._h, ptr(P0, C.c_float), ptr(P1, C.c_float), ptr(uv0, C.c_float),
                                       ptr(uv1, C.c_float), n, ptr(K, d), ptr(H0, d), ptr(H1, d)))

    def dlt_resident(self):
        self._ck(self._L.vo_dlt_resident(self._h))

    def dlt_fetch(self):
        n, B = self._dlt_n, self.batch
        X4, depth, reproj = np.zeros((B, 4, n), np.float32), np.zeros((B, n)), np.zeros((B, n))
        self._ck(self._L.vo_dlt_fetch(self._h, ptr(X4, C.c_float), ptr(depth, C.c_double), ptr(reproj, C.c_double)))
        return (self._out(X4), self._out(depth), self._out(reproj)) if self._dlt_stats else self._out(X4)

    # -- fused frame step ----------------------------------------------------------------------
    def set_graph_mode(self, on=True):
        self._ck(self._L.vo_set_graph_mode(self._h, 1 if on else 0))

    def set_side_stream(self, on=True):
        """re-detection + triangulation of the fused step on a side stream beside the bundle adjustment (True / 1, default) or in
        line (False / 0); 2 or "pipeline": three streams -- the bundle adjustment of frame t also runs beside the front end of
        frame t + 1 (two steps in flight)"""
        mode = 2 if on in (2, "pipeline") else (1 if on else 0)
        self._ck(self._L.vo_set_side_stream(self._h, mode))

    def step_layout(self):
        """-> {"layout": 0 | 1 | 2, "gate_groups": LM launch groups of frame t that precede the tracker launch of frame t + 1 (0: no gate),
        "reserved_cus": compute units the front-end stream leaves free} -- what vo_set_side_stream put into effect"""
        a, b, d = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._L.vo_step_layout(self._h, C.byref(a), C.byref(b), C.byref(d)))
        return {"layout": a.value, "gate_groups": b.value, "reserved_cus": d.value}

    def frame_step_resident(self, frame_idx, n_pts, do_dlt=True, do_ba=True, do_st=True, mask_radius=7,
                            klt=None, st=None, ba=None):
        """enqueue one whole frame (pyramid, KLT, DLT, BA, re-detection, result copies); async"""
        klt = klt if klt is not None else self.klt_params()
        st = st if st is not None else self.st_params()
        ba = ba if ba is not None else self.ba_params()
        self._klt_levels = klt.max_level + 1
        self._st_max_corners = st.max_corners
        self._ck(self._L.vo_frame_step_resident(self._h, int(frame_idx), int(n_pts), int(do_dlt), int(do_ba), int(do_st),
                                                int(mask_radius), C.byref(klt), C.byref(st), C.byref(ba)))
        # what each step in flight will hand back (up to two are in flight, and they need not carry the same stages)
        if not hasattr(self, "_step_cfgs"):
            self._step_cfgs = []
        self._step_cfgs.append((n_pts, do_dlt, do_ba, do_st))

    def frame_step_host(self, frames, n_pts, do_dlt=True, do_ba=True, do_st=True, mask_radius=7, klt=None, st=None, ba=None):
        """the same step with this frame's images handed over by the host, as the reference's loop does (pipeline.py:98,171-172):
        frames = one uint8 [h, w] array per sequence (a list / tuple of `batch` arrays, rows contiguous, a common row stride) or one
        [batch, h, w] array.  The upload runs on a copy stream beside the previous step's bundle adjustment.  Arrays over pinned memory
        (`VoContext.host_alloc`) must stay untouched until `frame_fetch` has returned this step; the arrays are kept referenced until then."""
        ptrs, stride, frames = frames if isinstance(frames, tuple) and len(frames) == 3 and isinstance(frames[1], int) else self.host_frames(frames)
        klt = klt if klt is not None else self.klt_params()
        st = st if st is not None else self.st_params()
        ba = ba if ba is not None else self.ba_params()
        self._klt_levels = klt.max_level + 1
        self._st_max_corners = st.max_corners
        self._ck(self._L.vo_frame_step_host(self._h, ptrs, int(stride), int(n_pts), int(do_dlt), int(do_ba), int(do_st),
                                            int(mask_radius), C.byref(klt), C.byref(st), C.byref(ba)))
        if not hasattr(self, "_step_cfgs"):
            self._step_cfgs = []
        self._step_cfgs.append((n_pts, do_dlt, do_ba, do_st))
        if not hasattr(self, "_host_refs"):
            self._host_refs = []
        self._host_refs.append(frames)          # released by frame_fetch: DMA out of pinned arrays is asynchronous
        while len(self._host_refs) > 2:
            self._host_refs.pop(0)


    def host_frames(self, frames):
        """-> (pointer array, row stride, the arrays): the checked form of one step's images that `frame_step_host` also accepts directly (a loader
        that cycles through a fixed set of buffers builds it once per buffer)"""
        if isinstance(frames, np.ndarray):
            frames = [frames] if frames.ndim == 2 else list(frames)
        if len(frames) != self.batch:
            raise ValueError("frame_step_host: %d frames for a batch of %d" % (len(frames), self.batch))
        stride = None
        ptrs = (C.c_void_p * self.batch)()
        for b, f in enumerate(frames):
            if f.dtype != np.uint8 or f.shape != (self.height, self.width) or f.strides[1] != 1 or f.strides[0] < self.width:
                raise ValueError("frame_step_host: expected uint8 [%d, %d] images with contiguous rows" % (self.height, self.width))
            if stride is None:
                stride = f.strides[0]
            elif f.strides[0] != stride:
                raise ValueError("frame_step_host: the images of a step share one row stride")
            ptrs[b] = f.ctypes.data
        return ptrs, int(stride), frames

    @classmethod
    def host_alloc(cls, shape, dtype=np.uint8):
        """numpy array over page-locked host memory (vo_host_alloc): what a loader decodes frames into so that `frame_step_host` uploads them
        by DMA without a staging copy.  Freed when the array (and every view of it) is gone."""
        import weakref
        L = _lib.load()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        rc = L.vo_host_alloc(max(n, 1), C.byref(p))
        if rc != 0:
            raise VoError(rc, "vo_host_alloc(%d bytes) failed" % n)
        buf = (C.c_uint8 * max(n, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        weakref.finalize(buf, L.vo_host_free, C.c_void_p(p.value)).atexit = False      # (at interpreter exit the process's memory goes anyway; the HIP runtime may be gone first)
        return arr

    def frame_fetch(self):
        """wait for the enqueued frame and return its results as a dict of numpy arrays"""
        if getattr(self, "_step_cfgs", None):
            self._step_cfg = self._step_cfgs.pop(0)          # the OLDEST step not fetched yet (nothing in flight: the last one again)
        n_pts, do_dlt, do_ba, do_st = self._step_cfg
        B = self.batch
        p, stt, err = np.zeros((B, n_pts, 2), np.float32), np.zeros((B, n_pts), np.uint8), np.zeros((B, n_pts), np.float32)
        X4 = depth = reproj = poses = points = corners = None
        bs = (BaStats * B)()
        nc = np.zeros(B, np.int32)
        if do_dlt:
            n = self._dlt_n
            X4, depth, reproj = np.zeros((B, 4, n), np.float32), np.zeros((B, n)), np.zeros((B, n))
        if do_ba:
            W, N = self._ba_shape
            poses, points = np.zeros((B, W, 6)), np.zeros((B, N, 3))
        mc = self._st_max_corners if self._st_max_corners > 0 else 4096
        if do_st:
            corners = np.zeros((B, mc, 2), np.float32)
        d = C.c_double
        self._ck(self._L.vo_frame_fetch(self._h, n_pts, ptr(p, C.c_float), ptr(stt, C.c_uint8), ptr(err, C.c_float),
                                        ptr(X4, C.c_float), ptr(depth, d), ptr(reproj, d), ptr(poses, d), ptr(points, d),
                                        bs, ptr(corners, C.c_float), ptr(nc, C.c_int32) if do_st else None))
        out = dict(points2d=self._out(p), status=self._out(stt), err=self._out(err))
        if do_dlt:
            out.update(X4=self._out(X4), depth1=self._out(depth), reproj=self._out(reproj))
        if do_ba:
            stats = [self._stats(bs[b]) for b in range(B)]
            out.update(poses=self._out(poses), landmarks=self._out(points), ba_stats=stats[0] if B == 1 else stats)
        if do_st:
            out["corners"] = self._corners(corners, nc)
        return out

    # -- in-stream timing -----------------------------------------------------------------------
    PROF_FRAME, PROF_KLT, PROF_ST, PROF_DLT, PROF_BA, PROF_CLAHE_LUT, PROF_CLAHE_APPLY = range(7)
    PROF_HOM_SOLVE, PROF_HOM_SCORE, PROF_HOM_SELECT, PROF_HOM_FINISH = range(7, 11)
    PROF_ORB_PYRAMID, PROF_ORB_CANDIDATES, PROF_ORB_RETAIN, PROF_ORB_DESCRIBE = range(11, 15)
    PROF_FUND_SOLVE, PROF_FUND_SCORE, PROF_FUND_SELECT, PROF_FUND_FINISH = range(15, 19)
    PROF_GMATCH_FORWARD, PROF_GMATCH_REVERSE, PROF_GMATCH_ACCEPT = range(19, 22)
    PROF_HPOSE = 22
    PROF_SIM3_SOLVE, PROF_SIM3_SCORE, PROF_SIM3_SELECT, PROF_SIM3_FINISH = range(23, 27)
    PROF_ALIGN = 27
    PROF_DEPTH = 28

    def profile_enable(self, regions=(0, 1, 2, 3, 4)):
        """regions: iterable of PROF_* ids to time with hipEvent pairs on the ctx stream; () switches timing off"""
        mask = 0
        for r in regions:
            mask |= 1 << r
        self._ck(self._L.vo_profile_enable(self._h, mask))

    def profile_read(self, region):
        t, n = C.c_double(0), C.c_int32(0)
        self._ck(self._L.vo_profile_read(self._h, region, C.byref(t), C.byref(n)))
        return t.value, n.value

    def debug_cycles(self, which):
        out = np.zeros(8, np.int64)
        self._ck(self._L.vo_debug_cycles(self._h, which, ptr(out, C.c_int64)))
        return out

    # -- BA -------------------------------------------------------------------------------------
    def ba_params(self, max_iters=50, ftol=1e-3, xtol=1e-3, gtol=1e-8, lambda0=1e-4, huber_delta=1.0, lambda_min=1e-3, loss='huber'):
        """loss: scipy's name ('huber', 'linear', 'soft_l1', 'cauchy', 'arctan'); huber_delta is scipy's f_scale for every loss"""
        p = BaParams()
        self._L.vo_ba_default_params(C.byref(p))
        p.max_iters, p.ftol, p.xtol, p.gtol, p.lambda0, p.huber_delta = max_iters, ftol, xtol, gtol, lambda0, huber_delta
        p.lambda_min = lambda_min
        p.loss = _lib.loss_code(loss)
        return p

    @staticmethod
    def _stats(s):
        return dict(cost0=s.cost0, cost=s.cost, lam=s.lam, iters=s.iters, accepted=s.accepted, status=s.status,
                    n_obs=s.n_obs)

    def _ba_inputs(self, K, poses, points, obs):
        obs = np.asarray(obs, np.float64)
        if self.batch == 1 and obs.ndim == 3:
            obs = obs[None]
        assert obs.ndim == 4 and obs.shape[0] == self.batch and obs.shape[3] == 2
        W, N = obs.shape[1:3]
        return (self._in(K, np.float64, (3, 3)), self._in(poses, np.float64, (W, 6)), self._in(points, np.float64, (N, 3)),
                np.ascontiguousarray(obs), W, N)

    def ba_adjust(self, K, poses, points, obs, params=None):
        """poses (W,6) [rvec,tvec; slot 0 newest], points (N,3), obs (W,N,2) NaN = unobserved.
        -> poses (W,6), points (N,3), stats dict   [leading batch dim / list of dicts if batch > 1]"""
        K, poses, points, obs, W, N = self._ba_inputs(K, poses, points, obs)
        B = self.batch
        prm = params if params is not None else self.ba_params()
        po, pt, st = np.zeros((B, W, 6)), np.zeros((B, N, 3)), (BaStats * B)()
        d = C.c_double
        self._ck(self._L.vo_ba_adjust(self._h, ptr(K, d), ptr(poses, d), ptr(points, d), ptr(obs, d), W, N, C.byref(prm),
                                      ptr(po, d), ptr(pt, d), st))
        self._ba_shape = (W, N)
        stats = [self._stats(st[b]) for b in range(B)]
        return self._out(po), self._out(pt), stats[0] if B == 1 else stats

    def ba_upload(self, K, poses, points, obs):
        K, poses, points, obs, W, N = self._ba_inputs(K, poses, points, obs)
        self._ba_shape = (W, N)
        d = C.c_double
        self._ck(self._L.vo_ba_upload(self._h, ptr(K, d), ptr(poses, d), ptr(points, d), ptr(obs, d), W, N))

    def ba_upload_bank(self, K, poses, points, obs):
        """a bank of resident problems of one shape: poses [n, B, W, 6], points [n, B, N, 3], obs [n, B, W, N, 2] (B = batch);
        ba_select(k) picks the one the next resident solve / frame step works on (no upload, no launch)"""
        obs = np.ascontiguousarray(obs, np.float64)
        n, B, W, N = obs.shape[:4]
        assert B == self.batch and obs.shape[4] == 2
        poses = np.ascontiguousarray(poses, np.float64).reshape(n, B, W, 6)
        points = np.ascontiguousarray(points, np.float64).reshape(n, B, N, 3)
        K = self._in(K, np.float64, (3, 3))
        d = C.c_double
        self._ck(self._L.vo_ba_upload_bank(self._h, ptr(K, d), ptr(poses, d), ptr(points, d), ptr(obs, d), W, N, n))
        self._ba_shape = (W, N)

    def ba_select(self, k):
        self._ck(self._L.vo_ba_select_problem(self._h, int(k)))

    def ba_solve_resident(self, params=None):
        prm = params if params is not None else self.ba_params()
        self._ck(self._L.vo_ba_solve_resident(self._h, C.byref(prm)))

    def ba_fetch(self):
        W, N = self._ba_shape
        B = self.batch
        po, pt, st = np.zeros((B, W, 6)), np.zeros((B, N, 3)), (BaStats * B)()
        self._ck(self._L.vo_ba_fetch(self._h, ptr(po, C.c_double), ptr(pt, C.c_double), st))
        stats = [self._stats(st[b]) for b in range(B)]
        return self._out(po), self._out(pt), stats[0] if B == 1 else stats

    def ba_fetch_after(self, solve, params):
        """solve(params) then ba_fetch() -- a resident solve whose result is wanted at once"""
        solve(params)
        return self.ba_fetch()

    # -- 3D-2D pose -----------------------------------------------------------------------------
    def pnp_ransac(self, K, pts3d, pts2d, reproj_err=2.0, confidence=0.9999, max_iters=1000000, seed=0):
        """RANSAC P3P + refinement.  pts3d (n,3), pts2d (n,2) [leading batch dim if batch > 1]
        -> rvec (3,), tvec (3,), inlier indices (ascending), stats dict   [lists / arrays over the batch]"""
        B = self.batch
        p3 = np.ascontiguousarray(pts3d, np.float32).reshape(B, -1, 3)
        p2 = np.ascontiguousarray(pts2d, np.float32).reshape(B, -1, 2)
        n = p3.shape[1]
        assert p2.shape[1] == n
        Kc = self._in(K, np.float64, (3, 3))
        prm = PnpParams()
        self._L.vo_pnp_default_params(C.byref(prm))
        prm.reproj_err, prm.confidence, prm.max_iters, prm.seed = reproj_err, confidence, int(max_iters), int(seed)
        rv, tv = np.zeros((B, 3)), np.zeros((B, 3))
        mask = np.zeros((B, n), np.uint8)
        st = (PnpStats * B)()
        self._ck(self._L.vo_pnp_ransac(self._h, ptr(Kc, C.c_double), ptr(p3, C.c_float), ptr(p2, C.c_float), n, C.byref(prm),
                                       ptr(rv, C.c_double), ptr(tv, C.c_double), ptr(mask, C.c_uint8), st))
        stats = [dict(cost=s.cost, n_inliers=s.n_inliers, hypotheses=s.hypotheses, best=s.best, status=s.status) for s in st]
        inl = [np.nonzero(mask[b])[0] for b in range(B)]
        if B == 1:
            return rv[0], tv[0], inl[0], stats[0]
        return rv, tv, inl, stats

    # -- SIFT ---------------------------------------------------------------------------------------
    def sift_detect_compute(self, img, mask=None, nfeatures=1000, max_out=None):
        """cv2.SIFT_create(nfeatures).detect(img, mask) + compute.  img (h, w) u8 [leading batch dim if batch > 1]
        -> keypoints (n, 6) float64 [x, y, size, angle, response, octave], descriptors (n, 128) float32   [lists over the batch]"""
        B = self.batch
        im = np.ascontiguousarray(img, np.uint8).reshape(B, self.height, self.width)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(B, self.height, self.width)
        cap = int(max_out) if max_out else (2 * nfeatures + 64 if nfeatures > 0 else 1 << 16)
        kps = (SiftKp * (B * cap))()
        desc = np.zeros((B, cap, 128), np.float32)
        n_out = np.zeros(B, np.int32)
        self._ck(self._L.vo_sift_detect_compute(self._h, ptr(im, C.c_uint8), self.width, None if mk is None else ptr(mk, C.c_uint8),
                                                int(nfeatures), cap, kps, ptr(desc, C.c_float), ptr(n_out, C.c_int32)))
        raw = np.frombuffer(kps, dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                                                 ("octave", "<i4")])).reshape(B, cap)
        outs = []
        for b in range(B):
            r = raw[b, :n_out[b]]
            k = np.stack([r["x"], r["y"], r["size"], r["angle"], r["response"], r["octave"]], 1).astype(np.float64).reshape(-1, 6)
            outs.append((k, desc[b, :n_out[b]].copy()))
        return outs[0] if B == 1 else outs

    # -- ORB ----------------------------------------------------------------------------------------
    def orb_params(self, nfeatures=500, scale_factor=1.2, nlevels=8, fast_threshold=20):
        p = OrbParams()
        self._L.vo_orb_default_params(C.byref(p))
        p.nfeatures, p.scale_factor, p.nlevels, p.fast_threshold = int(nfeatures), float(scale_factor), int(nlevels), int(fast_threshold)
        return p

    def orb_detect_compute(self, img, mask=None, nfeatures=500, scale_factor=1.2, nlevels=8, fast_threshold=20, pattern=None, max_out=None):
        """multi-scale ORB (vo_orb_detect_compute; the definition is tests/orb_model.py, not cv2.ORB).  img (h, w) u8 [leading batch dim if
        batch > 1], mask the same shape or None; pattern as in brief_compute -> keypoints (n,) structured [x, y, size, angle, response, octave,
        lx, ly] (_lib.ORB_KP_DTYPE), descriptors (n, 32) uint8   [lists over the batch].  max_out: output rows per sequence (default
        2 * nfeatures + 64, at most 65536); VoError VO_E_CAPACITY when a sequence has more."""
        B = self.batch
        im = np.ascontiguousarray(img, np.uint8).reshape(B, self.height, self.width)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(B, self.height, self.width)
        cap = int(max_out) if max_out is not None else min(2 * int(nfeatures) + 64, 1 << 16)
        prm = self.orb_params(nfeatures, scale_factor, nlevels, fast_threshold)
        pat = self._brief_pattern(pattern)
        n = max(cap, 1)
        kps = np.zeros((B, n), _lib.ORB_KP_DTYPE)
        desc = np.zeros((B, n, 32), np.uint8)
        n_out = np.zeros(B, np.int32)
        self._ck(self._L.vo_orb_detect_compute(self._h, ptr(im, C.c_uint8), self.width, None if mk is None else ptr(mk, C.c_uint8), C.byref(prm),
                                               ptr(pat, C.c_int8), cap, kps.ctypes.data_as(C.POINTER(OrbKp)), ptr(desc, C.c_uint8),
                                               ptr(n_out, C.c_int32)))
        outs = [(kps[b, :n_out[b]].copy(), desc[b, :n_out[b]].copy()) for b in range(B)]
        return outs[0] if B == 1 else outs

    def orb_levels(self):
        """the pyramid of the last orb_detect_compute (vo_orb_levels_read / vo_orb_level_image_read) -> dict(w_l, h_l, scale_l f32, quota_l: [8],
        zeros beyond nlevels; n_l (batch, 8): keypoints each level returned; images: per sequence, the level images (h_l, w_l) u8)"""
        w_l, h_l, q_l = np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros(8, np.int32)
        s_l, n_l = np.zeros(8, np.float32), np.zeros((self.batch, 8), np.int32)
        self._ck(self._L.vo_orb_levels_read(self._h, ptr(w_l, C.c_int32), ptr(h_l, C.c_int32), ptr(s_l, C.c_float), ptr(q_l, C.c_int32),
                                            ptr(n_l, C.c_int32)))
        nlevels = int(np.count_nonzero(s_l))
        images = []
        for b in range(self.batch):
            lv = []
            for l in range(nlevels):
                out = np.zeros((h_l[l], w_l[l]), np.uint8)
                self._ck(self._L.vo_orb_level_image_read(self._h, b, l, ptr(out, C.c_uint8)))
                lv.append(out)
            images.append(lv)
        return dict(w_l=w_l, h_l=h_l, scale_l=s_l, quota_l=q_l, n_l=n_l, nlevels=nlevels, images=images)

    # -- descriptor matching ----------------------------------------------------------------------
    def match_knn2(self, desc1, desc2):
        """two nearest train descriptors (L2) of every query descriptor.  desc1 (n1,dim), desc2 (n2,dim) f32
        [leading batch dim if batch > 1] -> idx (n1,2) int32 (-1 = none), dist (n1,2) float32"""
        B = self.batch
        dim = np.shape(desc1)[-1]
        d1 = np.ascontiguousarray(desc1, np.float32).reshape(B, -1, dim)
        d2 = np.ascontiguousarray(desc2, np.float32).reshape(B, -1, dim)
        n1, n2 = d1.shape[1], d2.shape[1]
        idx = np.zeros((B, n1, 2), np.int32); dist = np.zeros((B, n1, 2), np.float32)
        self._ck(self._L.vo_match_knn2(self._h, ptr(d1, C.c_float), n1, ptr(d2, C.c_float), n2, dim, ptr(idx, C.c_int32),
                                       ptr(dist, C.c_float)))
        return (idx[0], dist[0]) if B == 1 else (idx, dist)

    def match_hamming_knn2(self, desc1, desc2):
        """two nearest train descriptors under the bit distance of every query descriptor (vo_match_hamming_knn2;
        cv2.BFMatcher(NORM_HAMMING).knnMatch(k=2)).  desc1 (n1,nbytes), desc2 (n2,nbytes) u8, nbytes a multiple of 4 in 4..64
        [leading batch dim if batch > 1] -> idx (n1,2) int32 (-1 = none), dist (n1,2) int32 (INT32_MAX = none)"""
        B = self.batch
        nb = np.shape(desc1)[-1]
        d1 = np.ascontiguousarray(desc1, np.uint8).reshape(B, -1, nb)
        d2 = np.ascontiguousarray(desc2, np.uint8).reshape(B, -1, nb)
        n1, n2 = d1.shape[1], d2.shape[1]
        idx = np.zeros((B, n1, 2), np.int32); dist = np.zeros((B, n1, 2), np.int32)
        self._ck(self._L.vo_match_hamming_knn2(self._h, ptr(d1, C.c_uint8), n1, ptr(d2, C.c_uint8), n2, nb, ptr(idx, C.c_int32),
                                               ptr(dist, C.c_int32)))
        return (idx[0], dist[0]) if B == 1 else (idx, dist)

    def match_guided(self, desc1, desc2, pts1=None, pts2=None, F=None, centers=None, radius=None, epi_dist=None, ratio=1.0, max_dist=None,
                     cross_check=False, counts1=None, counts2=None):
        """guided matching (vo_match_guided_hamming for uint8 descriptors, vo_match_guided_l2 otherwise): the two nearest train rows of every
        query among the pairs a gate admits, and the accept rule on the device.  radius (pixels) sets the window gate: pts2[j] within radius of
        centers[i] (pts1[i] without centers); epi_dist (pixels) sets the epipolar gate under F (3,3), x2^T F x1 = 0: the pairs find_fundamental
        counts as inliers of F at that threshold.  ratio < 1: Lowe's test d0 < ratio d1; max_dist: d0 <= max_dist; cross_check: the match must be
        mutual.  desc1 (n1,w), desc2 (n2,w), pts1 / centers (n1,2), pts2 (n2,2) [leading batch dim if batch > 1]; counts1, counts2 (batch,):
        rows at or beyond a sequence's count do not exist.  -> dict match (n1,) train index or -1, idx (n1,2), dist (n1,2), n_admitted (n1,),
        rbest (n2,) the nearest admitted query of every train row under cross_check, else -1"""
        B = self.batch
        ham = np.asarray(desc1).dtype == np.uint8 and np.asarray(desc2).dtype == np.uint8
        dt, ct = (np.uint8, C.c_uint8) if ham else (np.float32, C.c_float)
        wd = np.shape(desc1)[-1]
        d1 = np.ascontiguousarray(desc1, dt).reshape(B, -1, wd)
        d2 = np.ascontiguousarray(desc2, dt).reshape(B, -1, wd)
        n1, n2 = d1.shape[1], d2.shape[1]

        def pos(p, n):
            return None if p is None else np.ascontiguousarray(p, np.float32).reshape(B, n, 2)

        def cnt(k):
            return None if k is None else np.ascontiguousarray(np.broadcast_to(np.asarray(k, np.int32).reshape(-1), (B,)), np.int32)
        p1, p2, ce = pos(pts1, n1), pos(pts2, n2), pos(centers, n1)
        Fm = None if F is None else np.ascontiguousarray(F, np.float64).reshape(B, 9)
        c1, c2 = cnt(counts1), cnt(counts2)
        prm = GMatchParams()
        self._L.vo_gmatch_default_params(C.byref(prm))
        prm.gate = (1 if radius is not None else 0) | (2 if epi_dist is not None else 0)
        prm.radius = 0.0 if radius is None else float(radius)
        prm.epi_dist = 0.0 if epi_dist is None else float(epi_dist)
        prm.ratio = float(ratio)
        if max_dist is not None:
            prm.max_dist = float(max_dist)
        prm.cross_check = int(cross_check)
        match = np.zeros((B, n1), np.int32); idx = np.zeros((B, n1, 2), np.int32)
        dist = np.zeros((B, n1, 2), np.int32 if ham else np.float32)
        nadm = np.zeros((B, n1), np.int32); rbest = np.zeros((B, n2), np.int32)
        fn = self._L.vo_match_guided_hamming if ham else self._L.vo_match_guided_l2
        self._ck(fn(self._h, ptr(d1, ct), n1, ptr(d2, ct), n2, wd, ptr(p1, C.c_float), ptr(p2, C.c_float), ptr(ce, C.c_float),
                    ptr(Fm, C.c_double), ptr(c1, C.c_int32), ptr(c2, C.c_int32), C.byref(prm), ptr(match, C.c_int32), ptr(idx, C.c_int32),
                    ptr(dist, C.c_int32 if ham else C.c_float), ptr(nadm, C.c_int32), ptr(rbest, C.c_int32)))
        out = dict(match=match, idx=idx, dist=dist, n_admitted=nadm, rbest=rbest)
        return {k: v[0] for k, v in out.items()} if B == 1 else out

    # -- 2D-2D bootstrap pose ---------------------------------------------------------------------
    def _two_views(self, pts1, pts2):
        """-> (p1, p2, n): the two views as C-contiguous [batch, n, 2] float32"""
        p1 = np.ascontiguousarray(pts1, np.float32).reshape(self.batch, -1, 2)
        p2 = np.ascontiguousarray(pts2, np.float32).reshape(self.batch, -1, 2)
        assert p2.shape[1] == p1.shape[1]
        return p1, p2, p1.shape[1]

    @staticmethod
    def _div33(*mats):
        """each [batch, 3, 3] in place: divided by its 3,3 entry as cv2 returns it, unless that is under 1e-12 of the norm"""
        for M in mats:
            for Mb in M:
                if abs(Mb[2, 2]) >= 1e-12 * np.linalg.norm(Mb):      # (False for NaN: left as it is)
                    Mb /= Mb[2, 2]

    def _inliers(self, mask):
        """mask [batch, n] -> the ascending inlier indices (a list of them per sequence if batch > 1)"""
        return self._out([np.nonzero(m)[0] for m in mask])

    def _hom_params(self, threshold, confidence, max_iters, seed, refine_iters):
        prm = HomParams()
        self._L.vo_homography_default_params(C.byref(prm))
        prm.threshold, prm.confidence, prm.max_iters, prm.seed, prm.refine_iters = threshold, confidence, int(max_iters), int(seed), int(refine_iters)
        return prm

    def _hom_stats(self, st):
        return self._out([dict(cost=s.cost, n_inliers=s.n_inliers, hypotheses=s.hypotheses, best=s.best, status=s.status, lm_iters=s.lm_iters) for s in st])

    def essential_ransac(self, K, pts1, pts2, threshold=1.0, prob=0.9999, max_iters=1000, seed=0, distance_thresh=50.0):
        """findEssentialMat(RANSAC) + recoverPose.  pts1, pts2 (n,2) pixels [leading batch dim if batch > 1]
        -> E (3,3) unit norm, R (3,3), t (3,) with x2 ~ R x1 + t, inlier indices (ascending), stats dict"""
        B = self.batch
        p1, p2, n = self._two_views(pts1, pts2)
        Kc = self._in(K, np.float64, (3, 3))
        prm = EssParams()
        self._L.vo_essential_default_params(C.byref(prm))
        prm.threshold, prm.prob, prm.distance_thresh, prm.max_iters, prm.seed = threshold, prob, distance_thresh, int(max_iters), int(seed)
        E, R, t = np.zeros((B, 3, 3)), np.zeros((B, 3, 3)), np.zeros((B, 3))
        mask = np.zeros((B, n), np.uint8)
        st = (EssStats * B)()
        self._ck(self._L.vo_essential_ransac(self._h, ptr(Kc, C.c_double), ptr(p1, C.c_float), ptr(p2, C.c_float), n, C.byref(prm),
                                             ptr(E, C.c_double), ptr(R, C.c_double), ptr(t, C.c_double), ptr(mask, C.c_uint8), st))
        stats = [dict(n_inliers=s.n_inliers, n_good=s.n_good, hypotheses=s.hypotheses, best=s.best, status=s.status) for s in st]
        return self._out(E), self._out(R), self._out(t), self._inliers(mask), self._out(stats)

    def find_homography(self, pts1, pts2, threshold=3.0, confidence=0.995, max_iters=2000, seed=0, refine_iters=10):
        """cv2.findHomography(pts1, pts2, cv2.RANSAC, threshold) (vo_homography_ransac).  pts1, pts2 (n,2) pixels, n >= 4 [leading batch dim
        if batch > 1] -> H (3,3) with x2 ~ H x1, re-fitted on the inliers and refined, inlier indices (ascending, the consensus set of H0),
        stats dict, H0 (3,3) the winning four-point sample's own model.  H and H0 are divided by h33 as cv2 returns them; where |h33| is under
        1e-12 of the norm they stay at unit Frobenius norm.  Without a model: stats['status'] != 0, NaN matrices, no inliers."""
        B = self.batch
        p1, p2, n = self._two_views(pts1, pts2)
        prm = self._hom_params(threshold, confidence, max_iters, seed, refine_iters)
        H, H0 = np.zeros((B, 3, 3)), np.zeros((B, 3, 3))
        mask = np.zeros((B, n), np.uint8)
        st = (HomStats * B)()
        self._ck(self._L.vo_homography_ransac(self._h, ptr(p1, C.c_float), ptr(p2, C.c_float), n, C.byref(prm), ptr(H, C.c_double),
                                              ptr(H0, C.c_double), ptr(mask, C.c_uint8), st))
        self._div33(H, H0)
        return self._out(H), self._inliers(mask), self._hom_stats(st), self._out(H0)

    def _hpose_params(self, ratio, threshold, min_off, normal_hint):
        prm = HposeParams()
        self._L.vo_homography_pose_default_params(C.byref(prm))
        prm.ratio, prm.threshold, prm.min_off = float(ratio), float(threshold), int(min_off)
        if normal_hint is not None:
            prm.use_hint = 1
            prm.hint[:] = [float(x) for x in np.asarray(normal_hint, np.float64).reshape(3)]
        return prm

    def _hpose_out(self, R, t, nrm, st):
        stats = [dict(n_solutions=s.n_solutions, n_distinct=s.n_distinct, ambiguous=s.ambiguous, status=s.status, n_mask=s.n_mask,
                      n_good=list(s.n_good), n_off=list(s.n_off), sigma=np.array(s.sigma), rotation_only=s.n_solutions == 1) for s in st]
        return self._out(R), self._out(t), self._out(nrm), self._out(stats)

    def decompose_homography(self, K, H, pts1=None, pts2=None, mask=None, ratio=0.75, threshold=1.0, min_off=8, normal_hint=None):
        """cv2.decomposeHomographyMat(H, K) with cv2.filterHomographyDecompByVisibleRefpoints' two visibility tests counted as votes, a ranking
        and an ambiguity verdict (vo_homography_decompose; the algorithm: tests/hpose_model.py).  K (3,3); H (3,3) with x2 ~ H x1 at any scale
        and sign; pts1, pts2 (n,2) pixels or None (the pure decomposition, every vote 0); mask (n,) nonzero = on the plane, None = every
        point [leading batch dim if batch > 1; one K serves every sequence].  threshold (px) is the Sampson threshold of the points outside
        the mask; normal_hint (3,) a plane-normal prior in view-1 camera coordinates.
        -> R (4,3,3), t (4,3) = t / d as cv2 returns it, n (4,3), best first, NaN beyond stats['n_solutions'] (4; 1 for a rotation-only H,
        then t = n = 0 and stats['rotation_only']; 0 with stats['status'] != 0 for an H without a solution), stats dict with n_distinct,
        ambiguous, n_mask, n_good, n_off (per ranked candidate), sigma."""
        B = self.batch
        Kc = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (B, 3, 3)))
        Hc = self._in(H, np.float64, (3, 3))
        p1 = p2 = m = None
        n = 0
        if pts1 is not None:
            p1, p2, n = self._two_views(pts1, pts2)
            if mask is not None:
                m = np.ascontiguousarray(np.asarray(mask).reshape(B, n) != 0, np.uint8)
        prm = self._hpose_params(ratio, threshold, min_off, normal_hint)
        R, t, nrm = np.zeros((B, 4, 3, 3)), np.zeros((B, 4, 3)), np.zeros((B, 4, 3))
        st = (HposeStats * B)()
        self._ck(self._L.vo_homography_decompose(self._h, ptr(Kc, C.c_double), ptr(Hc, C.c_double), ptr(p1, C.c_float), ptr(p2, C.c_float),
                                                 ptr(m, C.c_uint8), n, C.byref(prm), ptr(R, C.c_double), ptr(t, C.c_double),
                                                 ptr(nrm, C.c_double), st))
        return self._hpose_out(R, t, nrm, st)

    def homography_pose(self, K, pts1, pts2, threshold=3.0, confidence=0.995, max_iters=2000, seed=0, refine_iters=10, ratio=0.75,
                        pose_threshold=1.0, min_off=8, normal_hint=None):
        """find_homography(pts1, pts2, threshold, ...) and decompose_homography of its H against its inliers in one call
        (vo_homography_pose): the decomposition runs behind the search on the device, on the H and the mask where they lie; the result is
        that of the two calls, bit for bit.  pose_threshold is decompose_homography's threshold.
        -> H (3,3) divided by h33, inlier indices, the search's stats dict, then R, t, n, stats as decompose_homography returns them."""
        B = self.batch
        p1, p2, n = self._two_views(pts1, pts2)
        Kc = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (B, 3, 3)))
        hp = self._hom_params(threshold, confidence, max_iters, seed, refine_iters)
        prm = self._hpose_params(ratio, pose_threshold, min_off, normal_hint)
        H = np.zeros((B, 3, 3))
        mask = np.zeros((B, n), np.uint8)
        R, t, nrm = np.zeros((B, 4, 3, 3)), np.zeros((B, 4, 3)), np.zeros((B, 4, 3))
        hs, st = (HomStats * B)(), (HposeStats * B)()
        self._ck(self._L.vo_homography_pose(self._h, ptr(Kc, C.c_double), ptr(p1, C.c_float), ptr(p2, C.c_float), n, C.byref(hp), C.byref(prm),
                                            ptr(H, C.c_double), ptr(mask, C.c_uint8), ptr(R, C.c_double), ptr(t, C.c_double),
                                            ptr(nrm, C.c_double), hs, st))
        self._div33(H)
        return (self._out(H), self._inliers(mask), self._hom_stats(hs)) + self._hpose_out(R, t, nrm, st)

    def find_fundamental(self, pts1, pts2, threshold=3.0, confidence=0.99, max_iters=1000, seed=0, refit=0):
        """cv2.findFundamentalMat(pts1, pts2, cv2.FM_RANSAC, threshold, confidence) (vo_fundamental_ransac).  pts1, pts2 (n,2) pixels, n >= 7
        [leading batch dim if batch > 1] -> F (3,3) with x2^T F x1 = 0 (refit=0: the winning seven-point sample's model, as cv2 returns it;
        refit=1: the normalised eight-point re-fit on the inliers, rank 2), inlier indices (ascending, the consensus set of F0), stats dict,
        F0 (3,3) the winning sample's own model.  F and F0 are divided by f33 as cv2 returns them; where |f33| is under 1e-12 of the norm they
        stay at unit Frobenius norm.  Without a model: stats['status'] != 0, NaN matrices, no inliers."""
        B = self.batch
        p1, p2, n = self._two_views(pts1, pts2)
        prm = FundParams()
        self._L.vo_fundamental_default_params(C.byref(prm))
        prm.threshold, prm.confidence, prm.max_iters, prm.seed, prm.refit = threshold, confidence, int(max_iters), int(seed), int(refit)
        F, F0 = np.zeros((B, 3, 3)), np.zeros((B, 3, 3))
        mask = np.zeros((B, n), np.uint8)
        st = (FundStats * B)()
        self._ck(self._L.vo_fundamental_ransac(self._h, ptr(p1, C.c_float), ptr(p2, C.c_float), n, C.byref(prm), ptr(F, C.c_double),
                                               ptr(F0, C.c_double), ptr(mask, C.c_uint8), st))
        self._div33(F, F0)
        stats = [dict(cost=s.cost, n_inliers=s.n_inliers, hypotheses=s.hypotheses, best=s.best, status=s.status, n_roots=s.n_roots,
                      models=s.models) for s in st]
        return self._out(F), self._inliers(mask), self._out(stats), self._out(F0)

    def _two_sets(self, src, dst):
        """-> (src, dst, n): two sets of 3-D points as C-contiguous [batch, n, 3] float32"""
        a = np.ascontiguousarray(src, np.float32).reshape(self.batch, -1, 3)
        b = np.ascontiguousarray(dst, np.float32).reshape(self.batch, -1, 3)
        assert a.shape[1] == b.shape[1]
        return a, b, a.shape[1]

    def _sim3_stats(self, st):
        return self._out([dict(cost=s.cost, n_inliers=s.n_inliers, hypotheses=s.hypotheses, best=s.best, status=s.status,
                               degenerate=s.degenerate, refit=s.refit) for s in st])

    def estimate_sim3(self, src, dst, threshold=3.0, confidence=0.99, max_iters=1000, seed=0, with_scale=True, refit=1):
        """The similarity (with_scale=False: rigid motion) dst ~ s R src + t between two sets of corresponding 3-D points with outliers
        (vo_sim3_ransac; the algorithm: tests/sim3_model.py): three-point RANSAC with Umeyama's closed form, cv2.estimateAffine3D's
        threshold (in dst's units) and confidence.  src, dst (n,3), n >= 3 [leading batch dim if batch > 1]
        -> s (float; (batch,) if batch > 1), R (3,3), t (3,) -- refit=1: Umeyama over the consensus set, refit=0 or a degenerate set: the
        winning sample's model; stats['refit'] says which -- inlier indices (ascending, the consensus set of model0), stats dict, model0
        (13,) = (s, R row-major, t) of the winning sample.  Without a model: stats['status'] != 0, NaN outputs, no inliers."""
        B = self.batch
        a, b, n = self._two_sets(src, dst)
        prm = Sim3Params()
        self._L.vo_sim3_default_params(C.byref(prm))
        prm.threshold, prm.confidence, prm.max_iters, prm.seed = threshold, confidence, int(max_iters), int(seed)
        prm.with_scale, prm.refit = int(with_scale), int(refit)
        s, R, t, m0 = np.zeros(B), np.zeros((B, 3, 3)), np.zeros((B, 3)), np.zeros((B, 13))
        mask = np.zeros((B, n), np.uint8)
        st = (Sim3Stats * B)()
        self._ck(self._L.vo_sim3_ransac(self._h, ptr(a, C.c_float), ptr(b, C.c_float), n, C.byref(prm), ptr(s, C.c_double), ptr(R, C.c_double),
                                        ptr(t, C.c_double), ptr(m0, C.c_double), ptr(mask, C.c_uint8), st))
        return self._out(s), self._out(R), self._out(t), self._inliers(mask), self._sim3_stats(st), self._out(m0)

    def fit_sim3(self, src, dst, mask=None, with_scale=True):
        """Umeyama's least-squares alignment dst ~ s R src + t over the rows of `mask` ((n,), nonzero = use; None: every row) whose
        coordinates are finite, without a search (vo_sim3_fit).  On the inliers estimate_sim3 returned it gives that call's (s, R, t) bit
        for bit.  -> s, R (3,3), t (3,), stats dict [leading batch dim if batch > 1]; fewer than 3 rows or a collinear set:
        stats['status'] != 0 and NaN outputs."""
        B = self.batch
        a, b, n = self._two_sets(src, dst)
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask).reshape(B, n) != 0, np.uint8)
        s, R, t = np.zeros(B), np.zeros((B, 3, 3)), np.zeros((B, 3))
        st = (Sim3Stats * B)()
        self._ck(self._L.vo_sim3_fit(self._h, ptr(a, C.c_float), ptr(b, C.c_float), ptr(m, C.c_uint8), n, int(with_scale), ptr(s, C.c_double),
                                     ptr(R, C.c_double), ptr(t, C.c_double), st))
        return self._out(s), self._out(R), self._out(t), self._sim3_stats(st)

    def align_params(self, max_level=-1, min_level=0, max_iters=10, min_points=10, huber=10.0, eps=1e-5, form=0):
        """vo_align_params: max_level -1 = the store's top level; huber in grey levels (0: no weighting); form 0 = the library's rule,
        1 = reference patches kept in a workspace, 2 = recomputed every iteration (the same bits)"""
        p = AlignParams()
        self._L.vo_align_default_params(C.byref(p))
        p.max_level, p.min_level, p.max_iters, p.min_points = int(max_level), int(min_level), int(max_iters), int(min_points)
        p.huber, p.eps, p.form = huber, eps, int(form)
        return p

    def sparse_align(self, K, pts3d, rvec0=None, tvec0=None, params=None):
        """Sparse direct image alignment (vo_sparse_align; the algorithm: tests/align_model.py): the pose of the store's current frame against
        its previous one from the two pyramids and pts3d (n,3), points in the PREVIOUS camera's coordinates (a NaN row or z <= 0 is never
        used) -- available before any feature is tracked.  K (3,3); rvec0 / tvec0 (3,): the initial pose, both None = identity [leading
        batch dim if batch > 1] -> rvec (3,), tvec (3,) with x_cur = R(rvec) x_prev + tvec, used (n,) bool (the points of the last kept
        linearisation of the finest level that ran), stats dict.  No level ran: stats['status'] != 0 and the initial pose comes back."""
        B = self.batch
        X = np.ascontiguousarray(pts3d, np.float32).reshape(B, -1, 3)
        n = X.shape[1]
        Kc = self._in(K, np.float64, (3, 3))
        if (rvec0 is None) != (tvec0 is None):
            raise ValueError("rvec0 and tvec0 go together")
        r0 = None if rvec0 is None else self._in(rvec0, np.float64, (3,))
        t0 = None if tvec0 is None else self._in(tvec0, np.float64, (3,))
        prm = params if params is not None else self.align_params()
        rv, tv = np.zeros((B, 3)), np.zeros((B, 3))
        mask = np.zeros((B, n), np.uint8)
        st = (AlignStats * B)()
        self._ck(self._L.vo_sparse_align(self._h, ptr(Kc, C.c_double), ptr(X, C.c_float), n, ptr(r0, C.c_double), ptr(t0, C.c_double), C.byref(prm),
                                         ptr(rv, C.c_double), ptr(tv, C.c_double), ptr(mask, C.c_uint8), st))
        stats = [dict(status=s.status, n_used=s.n_used, levels_run=s.levels_run, flags=s.flags, iters=list(s.iters), chi2=s.chi2, zbar=s.zbar)
                 for s in st]
        return self._out(rv), self._out(tv), self._out(mask != 0), self._out(stats)

    def depth_params(self, max_steps=128, max_iters=10, max_score=300 * 64, eps_align=0.03, px_noise=1.0, conv_ratio=200.0, min_inlier=0.1):
        """vo_depth_params: max_steps the longest epipolar segment searched (pixels, 1..128); max_score the largest ZMSSD sum of a match;
        eps_align / px_noise in pixels; converged at sqrt(sigma2) < z_range / conv_ratio, diverged at a / (a + b) < min_inlier"""
        p = DepthParams()
        self._L.vo_depth_default_params(C.byref(p))
        p.max_steps, p.max_iters, p.max_score = int(max_steps), int(max_iters), int(max_score)
        p.eps_align, p.px_noise, p.conv_ratio, p.min_inlier = eps_align, px_noise, conv_ratio, min_inlier
        return p

    def depth_seeds(self, uv, depth_mean, depth_min, ref_id=0):
        """Depth-filter seeds at the pixels uv (n,2) of the store's CURRENT frame (vo_depth_seed_init; the algorithm:
        tests/depth_model.py): inverse distance 1 / depth_mean with a standard deviation of a sixth of 1 / depth_min, and the 10 x 10
        patches around the pixels.  depth_mean, depth_min: scalars (or (batch,)); ref_id: the row of depth_update's poses the seeds
        refer to [leading batch dim if batch > 1] -> DepthSeeds (.seeds a structured array (n,), .patches (n,100) u8, .ok (n,) bool:
        False where the patch leaves the image or the pixel is not finite; such a seed is flagged diverged)"""
        B = self.batch
        p = np.ascontiguousarray(uv, np.float32).reshape(B, -1, 2)
        n = p.shape[1]
        dm = np.ascontiguousarray(np.broadcast_to(np.asarray(depth_mean, np.float64).reshape(-1), (B,)))
        dn = np.ascontiguousarray(np.broadcast_to(np.asarray(depth_min, np.float64).reshape(-1), (B,)))
        seeds = np.zeros((B, n), _lib.DEPTH_SEED_DTYPE)
        patches, ok = np.zeros((B, n, 100), np.uint8), np.zeros((B, n), np.uint8)
        self._ck(self._L.vo_depth_seed_init(self._h, ptr(p, C.c_float), n, ptr(dm, C.c_double), ptr(dn, C.c_double), int(ref_id),
                                            seeds.ctypes.data_as(C.POINTER(DepthSeed)), ptr(patches, C.c_uint8), ptr(ok, C.c_uint8)))
        return DepthSeeds(self._out(seeds), self._out(patches), self._out(ok != 0))

    def depth_update(self, K, poses, seeds, params=None):
        """One depth-filter update of `seeds` (a DepthSeeds) against the store's CURRENT frame (vo_depth_update): a patch search along each
        seed's epipolar segment, sub-pixel alignment, triangulation and the Gaussian x Beta update.  K (3,3); poses (n_ref,6) rvec, tvec
        of x_cur = R x_ref + t, row seeds['ref_id'] for each seed [leading batch dim if batch > 1].  seeds.seeds is updated in place
        -> result (n,) u8 (an index into DEPTH_RESULTS), match_uv (n,2) f32, z (n,) f64 (NaN where there is none), stats dict (counts
        by result name, converged, diverged; a list of them if batch > 1)"""
        B = self.batch
        Kc = np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float64).reshape(-1, 3, 3), (B, 3, 3)))
        po = np.ascontiguousarray(poses, np.float64).reshape(B, -1, 6)
        s = seeds.seeds.reshape(B, -1)
        if not (s.flags["C_CONTIGUOUS"] and s.flags["WRITEABLE"] and np.shares_memory(s, seeds.seeds)):
            raise ValueError("seeds.seeds must be a contiguous, writable array")
        n = s.shape[1]
        pt = np.ascontiguousarray(seeds.patches, np.uint8).reshape(B, n, 100)
        prm = params if params is not None else self.depth_params()
        res, match, z = np.zeros((B, n), np.uint8), np.zeros((B, n, 2), np.float32), np.zeros((B, n))
        st = (DepthStats * B)()
        self._ck(self._L.vo_depth_update(self._h, ptr(Kc, C.c_double), ptr(po, C.c_double), po.shape[1], s.ctypes.data_as(C.POINTER(DepthSeed)),
                                         ptr(pt, C.c_uint8), n, C.byref(prm), ptr(res, C.c_uint8), ptr(match, C.c_float), ptr(z, C.c_double), st))
        stats = [dict(dict(zip(_lib.DEPTH_RESULTS, list(x.counts))), converged=x.converged, diverged=x.diverged) for x in st]
        return self._out(res), self._out(match), self._out(z), self._out(stats)

    def pnp_params(self, reproj_err=2.0, confidence=0.9999, max_iters=1000000, seed=0):
        prm = PnpParams()
        self._L.vo_pnp_default_params(C.byref(prm))
        prm.reproj_err, prm.confidence, prm.max_iters, prm.seed = reproj_err, confidence, int(max_iters), int(seed)
        return prm

    def pnp_upload(self, K, pts3d, pts2d):
        B = self.batch
        p3 = np.ascontiguousarray(pts3d, np.float32).reshape(B, -1, 3)
        p2 = np.ascontiguousarray(pts2d, np.float32).reshape(B, -1, 2)
        self._pnp_n = p3.shape[1]
        Kc = self._in(K, np.float64, (3, 3))
        self._ck(self._L.vo_pnp_upload(self._h, ptr(Kc, C.c_double), ptr(p3, C.c_float), ptr(p2, C.c_float), self._pnp_n))

    def pnp_solve_resident(self, params=None, blind_batches=2):
        prm = params if params is not None else self.pnp_params()
        self._ck(self._L.vo_pnp_solve_resident(self._h, C.byref(prm), int(blind_batches)))

    def pnp_fetch(self):
        B, n = self.batch, self._pnp_n
        rv, tv, mask, st = np.zeros((B, 3)), np.zeros((B, 3)), np.zeros((B, n), np.uint8), (PnpStats * B)()
        self._ck(self._L.vo_pnp_fetch(self._h, ptr(rv, C.c_double), ptr(tv, C.c_double), ptr(mask, C.c_uint8), st))
        stats = [dict(cost=s.cost, n_inliers=s.n_inliers, hypotheses=s.hypotheses, best=s.best, status=s.status) for s in st]
        inl = [np.nonzero(mask[b])[0] for b in range(B)]
        if B == 1:
            return rv[0], tv[0], inl[0], stats[0]
        return rv, tv, inl, stats

    # -- device-resident track table ------------------------------------------------------------
    def tracks_seed(self, pts, t=0):
        """Initial tracks born at frame t; pts (n,2) [(B,n,2)]."""
        pts, n = self._npts(pts)
        self._ck(self._L.vo_tracks_seed(self._h, ptr(pts, C.c_float), n, int(t)))

    def tracks_track(self, t, params=None):
        """KLT prev -> cur of every live track + the reference's pruning / bookkeeping (async)."""
        prm = params if params is not None else self.klt_params()
        self._ck(self._L.vo_tracks_track(self._h, int(t), C.byref(prm)))

    def tracks_detect(self, t, mask_radius=7, params=None, max_new=1000):
        """Shi-Tomasi re-detection around the live tracks; corners become tracks born at t (async)."""
        prm = params if params is not None else self.st_params()
        self._corner_slots = prm.max_corners if 0 < prm.max_corners < 4096 else 4096
        self._ck(self._L.vo_tracks_detect(self._h, int(t), int(mask_radius), C.byref(prm), int(max_new)))

    def tracks_read(self):
        """-> list (one dict per sequence; a dict if batch == 1) of uv, uv_first (n,2) f32, t_first, t_total, tag (n,),
        dead_tag (n_dead,)."""
        B, cap = self.batch, self.max_pts
        n, nd = np.zeros(B, np.int32), np.zeros(B, np.int32)
        uv, uf = np.zeros((B, cap, 2), np.float32), np.zeros((B, cap, 2), np.float32)
        tf, tt, tag, dead = (np.zeros((B, cap), np.int32) for _ in range(4))
        i, f = C.c_int32, C.c_float
        self._ck(self._L.vo_tracks_read(self._h, ptr(n, i), ptr(uv, f), ptr(uf, f), ptr(tf, i), ptr(tt, i), ptr(tag, i),
                                        ptr(nd, i), ptr(dead, i)))
        out = [dict(uv=uv[b, :n[b]].copy(), uv_first=uf[b, :n[b]].copy(), t_first=tf[b, :n[b]].copy(),
                    t_total=tt[b, :n[b]].copy(), tag=tag[b, :n[b]].copy(), dead_tag=dead[b, :nd[b]].copy()) for b in range(B)]
        return out[0] if B == 1 else out

    def tracks_counts(self):
        """-> (n_live, n_dead) per sequence [(B,) int32 each; ints if batch == 1]: the synchronous read-back of the counters only
        (vo_tracks_read with NULL tables) -- what a per-frame loop needs when the tables stay on the device"""
        B = self.batch
        n, nd = np.zeros(B, np.int32), np.zeros(B, np.int32)
        i = C.c_int32
        self._ck(self._L.vo_tracks_read(self._h, ptr(n, i), None, None, None, None, None, ptr(nd, i), None))
        return (int(n[0]), int(nd[0])) if B == 1 else (n, nd)

    def tracks_obs(self, t_now, window):
        """BA observation table of the live tracks -> (B, window, max_pts, 2) f64 [(window, max_pts, 2) if batch == 1]."""
        obs = np.zeros((self.batch, window, self.max_pts, 2))
        self._ck(self._L.vo_tracks_obs(self._h, int(t_now), int(window), ptr(obs, C.c_double)))
        return obs[0] if self.batch == 1 else obs

    def ba_obs_from_tracks(self, t_now):
        """Fill the observation table of the resident BA problem (N = max_pts, W slots) from the track ring (async)."""
        self._ck(self._L.vo_ba_obs_from_tracks(self._h, int(t_now)))

    # -- landmark-sharded BA of one problem (config 5) -------------------------------------------
    @staticmethod
    def comm_unique_id():
        """128-byte RCCL id (rank 0 makes it, every rank passes it to comm_init)."""
        L = _lib.load()
        uid = np.zeros(128, np.uint8)
        rc = L.vo_comm_unique_id(ptr(uid, C.c_uint8))
        if rc != 0:
            raise RuntimeError("vo_comm_unique_id failed (%d): librccl not loadable?" % rc)
        return uid

    def comm_init(self, n_ranks, rank, uid):
        uid = np.ascontiguousarray(uid, np.uint8)
        assert uid.size == 128
        self._ck(self._L.vo_comm_init(self._h, int(n_ranks), int(rank), ptr(uid, C.c_uint8)))
        self.comm_ranks, self.comm_rank = int(n_ranks), int(rank)

    def comm_destroy(self):
        self._ck(self._L.vo_comm_destroy(self._h))
        self.comm_ranks, self.comm_rank = 1, 0

    def ba_set_sharded(self, on=True):
        """The `batch` problems of ba_upload / ba_adjust (x the ranks of the communicator) are landmark shards of
        ONE problem (see sharding.shard_problem)."""
        self._ck(self._L.vo_ba_set_sharded(self._h, 1 if on else 0))

    def ba_gather_points(self):
        """-> points of every shard of every rank, (n_ranks, batch, N, 3)."""
        W, N = self._ba_shape
        R = getattr(self, "comm_ranks", 1)
        out = np.zeros((R, self.batch, N, 3))
        self._ck(self._L.vo_ba_gather_points(self._h, ptr(out, C.c_double)))
        return out

    def ba_probe(self, lam=1e-4, huber_delta=1.0, loss='huber'):
        """Parity probe of problem 0 at the uploaded x0: residuals, normal equations, reduced system, one LM step.
        loss: scipy's name, huber_delta its f_scale."""
        W, N = self._ba_shape
        res = np.zeros(W * N)
        n_obs = C.c_int32(0)
        cost = C.c_double(0)
        Hpp, gp = np.zeros((W, 6, 6)), np.zeros((W, 6))
        Hll, gl = np.zeros((N, 3, 3)), np.zeros((N, 3))
        S, rhs = np.zeros((6 * W, 6 * W)), np.zeros(6 * W)
        dp, dl = np.zeros((W, 6)), np.zeros((N, 3))
        d = C.c_double
        self._ck(self._L.vo_ba_probe_loss(self._h, lam, _lib.loss_code(loss), huber_delta, ptr(res, d), C.byref(n_obs), C.byref(cost),
                                     ptr(Hpp, d), ptr(gp, d), ptr(Hll, d), ptr(gl, d), ptr(S, d), ptr(rhs, d),
                                     ptr(dp, d), ptr(dl, d)))
        return dict(residual=res[:n_obs.value].copy(), cost=cost.value, Hpp=Hpp, gp=gp, Hll=Hll, gl=gl, S=S, rhs=rhs,
                    dposes=dp, dpoints=dl)
