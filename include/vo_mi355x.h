/*
 * vo_mi355x.h -- C ABI of libvo_mi355x.so: the MI355X (gfx950) visual-odometry inner loop.
 *
 * The reference (JonasFrey96/Visual-Odom-Pipeline) is pure Python and has no FFI; its hot path
 * sits behind two Python classes and bottoms out in OpenCV / SciPy calls.  This header declares
 * the flat entry points a ctypes binding uses to replace exactly those calls.  Every export cites
 * the reference call site it replaces (paths relative to /root/reference).  INTEGRATION.md shows
 * the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns int32_t: VO_OK (0) or a negative VO_E_* code; vo_last_error(ctx)
 *     gives the message.  No C++ exception crosses the boundary.
 *   - the caller owns all host buffers (C-contiguous numpy arrays); the library owns only the
 *     device memory inside the opaque vo_ctx.  One vo_ctx = one GPU + one HIP stream; calls on
 *     one ctx must be serialised by the caller; different ctxs are independent.
 *   - synchronous entry points return with the outputs written.  The *_async / *_resident forms
 *     only enqueue work on the ctx's stream; vo_sync() waits for it.
 *   - there is NO CPU fallback: without a HIP device vo_ctx_create fails with VO_E_HIP.
 */
#ifndef VO_MI355X_H
#define VO_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VO_ABI_VERSION 4

enum {
  VO_OK = 0,
  VO_E_INVALID = -1,     /* bad argument */
  VO_E_HIP = -2,         /* HIP runtime error / no device */
  VO_E_NOMEM = -3,
  VO_E_STATE = -4,       /* call sequence error (e.g. tracking before two frames were pushed) */
  VO_E_CAPACITY = -5,    /* a fixed-capacity device buffer would overflow */
  VO_E_NUMERIC = -6      /* solver breakdown (non-positive pivot, non-finite cost) */
};

typedef struct vo_ctx vo_ctx;

/* ---- parameters (defaults = the reference's hard-coded values) ------------------------------ */

/* cv2.calcOpticalFlowPyrLK parameters, src/extractor/extractor.py:16-19 */
typedef struct {
  int32_t win;               /* 31  (winSize 31x31; odd, <= 31)                     */
  int32_t max_level;         /* 3   (=> 4 pyramid levels)                            */
  int32_t max_count;         /* 30  TERM_CRITERIA_COUNT                              */
  double  epsilon;           /* 0.03 TERM_CRITERIA_EPS (squared internally)          */
  float   min_eig_threshold; /* 1e-4 (OpenCV default)                                */
  int32_t _pad;
} vo_klt_params;

/* cv2.goodFeaturesToTrack parameters, src/extractor/extractor.py:21-24 */
typedef struct {
  int32_t max_corners;       /* 1000 */
  int32_t block_size;        /* 31   */
  double  quality_level;     /* 0.03 */
  double  min_distance;      /* min_kp_dist (7 in src/pipeline/pipeline.py:21,27) */
  int32_t use_harris;        /* 0: cv2.goodFeaturesToTrack's default response, the minimum eigenvalue (what the reference runs: its parameter
                                dict extractor.py:21-24 leaves useHarrisDetector at False); 1: useHarrisDetector=True -- the response becomes
                                a c - b^2 - harris_k (a + c)^2 over the same box-filtered Sobel products without the 1/2 factors
                                (imgproc/corner.cpp calcHarris, its SCALAR form: float a c - b^2, the k term in double; a SIMD build of
                                cv2 evaluates all but the last pixels of a row in float throughout and differs by ~1 ulp -- parity is with
                                oracle/vo_oracle.c's restatement, not with cv2 bit for bit), everything after
                                the response map is unchanged.
                                A frame whose largest masked response is not positive yields no corners here (OpenCV would rank negative
                                responses). */
  int32_t fast_threshold;    /* 0: the response above (the default; what every caller that leaves the field alone gets, bit for bit).
                                1..254: the response is the FAST-9/16 corner score at threshold t = fast_threshold, what
                                cv2.FastFeatureDetector_create(t, True, TYPE_9_16) reports as a keypoint's `response`: with d_k the 16 differences
                                ring pixel - centre on the radius-3 circle, m = max over the 16 arcs of 9 consecutive k of
                                max(min d, min -d); a pixel at least 3 from every border with m > t scores m - 1 (the largest threshold at
                                which it still passes the segment test), every other pixel 0.  block_size (still validated), use_harris and
                                harris_k play no part; the mask, the quality threshold, the 3 x 3 >= test, the rank order (value, then pixel
                                index, both descending -- scores are small integers, ties are the rule) and the min-distance pass are unchanged.
                                Parity is with tests/fast_model.py, compared with a live cv2 where one is importable.
                                Outside 0..254, or > 0 together with use_harris: VO_E_INVALID, nothing enqueued. */
  double  harris_k;          /* 0.04 (OpenCV default) */
} vo_st_params;

/* Robust loss of the bundle adjustment, scipy.optimize.least_squares' names (vo_ba_params.loss).  With C = f_scale (huber_delta),
 * s = |e|^2 the squared pixel error of an observation and z = s / C^2, the cost is 1/2 C^2 sum rho(z) and the IRLS weight w = rho'(z):
 *   HUBER    z if z <= 1, else 2 sqrt(z) - 1          w = 1 or 1 / sqrt(z)
 *   LINEAR   z                                         w = 1   (runs the Huber kernels with an unreachable knee; C plays no part)
 *   SOFT_L1  2 (sqrt(1 + z) - 1)                       w = 1 / sqrt(1 + z)
 *   CAUCHY   log1p(z)                                  w = 1 / (1 + z)
 *   ARCTAN   atan(z)                                   w = 1 / (1 + z^2)
 * The Jacobians, the Schur complement, the Cholesky factorisation and the LM logic are the same for every loss; SOFT_L1, CAUCHY and ARCTAN
 * run their own instances of the loss-templated kernels (k_ba_build_w / k_ba_update_w, k_ba_build / k_ba_update).  scipy's rho''
 * rescaling of the Jacobian is not copied: the IRLS fixed point sum w J^T e = 0 is the point scipy's TRF converges to. */
enum {
  VO_LOSS_HUBER = 0,         /* the default: a zero-filled vo_ba_params is the reference's loss */
  VO_LOSS_LINEAR = 1,
  VO_LOSS_SOFT_L1 = 2,
  VO_LOSS_CAUCHY = 3,
  VO_LOSS_ARCTAN = 4
};

/* BundleAdjuster configuration, src/bundle_adjuster/bundle_adjuster.py:8-16 and
 * src/pipeline/pipeline.py:28-29 (xtol = ftol = 1e-3, loss 'huber', f_scale 1).
 * Every entry point that takes it (vo_ba_adjust, vo_ba_solve_resident, vo_frame_step*, vo_pipe_create / vo_pipe_params.ba) returns
 * VO_E_INVALID with nothing enqueued for an unknown loss code or a huber_delta that is <= 0 or NaN, and for SOFT_L1, CAUCHY and ARCTAN
 * a huber_delta outside [VO_BA_F_SCALE_MIN, VO_BA_F_SCALE_MAX] (+inf included), where C^2 or 1 / C^2 would overflow. */
#define VO_BA_F_SCALE_MIN 1e-150
#define VO_BA_F_SCALE_MAX 1e150
typedef struct {
  int32_t max_iters;         /* LM iterations (linearise + solve + evaluate) cap, e.g. 50 */
  int32_t loss;              /* VO_LOSS_*, default VO_LOSS_HUBER (0) */
  double  ftol;              /* 1e-3 */
  double  xtol;              /* 1e-3 */
  double  gtol;              /* 1e-8 (scipy default) */
  double  lambda0;           /* initial Marquardt damping, 1e-4 */
  double  huber_delta;       /* scipy's f_scale C for every loss (the name is the Huber knee's), 1.0 px */
  double  lambda_min;        /* floor of the damping, 1e-3.  The reference fixes no gauge, so the normal equations
                                have a 7-dimensional near-null space; without a floor the Nielsen schedule drives
                                lambda to ~1e-5 after two good steps and then spends 4-6 iterations on rejected
                                steps along the gauge directions before it has doubled its way back. */
} vo_ba_params;

typedef struct {
  double  cost0;             /* 0.5 * sum rho(|e|^2) at the input */
  double  cost;              /* at the output */
  double  lambda;            /* final damping */
  int32_t iters;             /* LM iterations executed */
  int32_t accepted;          /* accepted steps */
  int32_t status;            /* 1 gtol, 2 ftol, 3 xtol, 0 max_iters, 4 damping overflow, <0 VO_E_* */
  int32_t n_obs;
} vo_ba_stats;

/* cv2.solvePnPRansac parameters as Extractor.camera_pose passes them (src/extractor/extractor.py:182-185;
 * reprojectionError = max_err_reproj = 2.0 from src/pipeline/pipeline.py:124-125) */
typedef struct {
  double  reproj_err;        /* 2.0 px: consensus threshold on the reprojection error */
  double  confidence;        /* 0.9999 */
  int32_t max_iters;         /* 1000000 */
  int32_t seed;              /* of the counter-based sample generator (OpenCV: fixed RNG state) */
} vo_pnp_params;

typedef struct {
  double  cost;              /* sum of squared pixel errors over the consensus set after refinement */
  int32_t n_inliers;
  int32_t hypotheses;        /* evaluated */
  int32_t best;              /* index of the winning hypothesis */
  int32_t status;            /* 0, or VO_E_NUMERIC when no pose with >= 4 inliers was found */
} vo_pnp_stats;

/* cv2.findEssentialMat(p1, p2, K, prob=0.9999, method=RANSAC, threshold=1.0) + cv2.recoverPose(E, p1, p2, K) as
 * Extractor.camera_pose(corr='2D-2D') calls them (src/extractor/extractor.py:162-172) */
typedef struct {
  double  threshold;         /* 1.0 px: consensus threshold on the Sampson distance (divided by (fx + fy) / 2 internally) */
  double  prob;              /* 0.9999 */
  double  distance_thresh;   /* 50: recoverPose keeps triangulated depths in (0, distance_thresh) baselines */
  int32_t max_iters;         /* 1000 (OpenCV's default bound for findEssentialMat) */
  int32_t seed;              /* of the counter-based sample generator */
} vo_ess_params;

typedef struct {
  int32_t n_inliers;         /* consensus set of the returned E */
  int32_t n_good;            /* inliers in front of both cameras for the returned (R, t) */
  int32_t hypotheses;        /* five-point samples evaluated */
  int32_t best;              /* index of the winning sample */
  int32_t status;            /* 0, or VO_E_NUMERIC when no model with >= 5 inliers was found */
  int32_t pad;
} vo_ess_stats;

/* cv2.findHomography(p1, p2, cv2.RANSAC, ransacReprojThreshold=3.0, maxIters=2000, confidence=0.995): the model the reference's bootstrap
 * names and never fits (src/pipeline/pipeline.py:66, "Estimate homography") */
typedef struct {
  double  threshold;         /* 3.0 px: consensus threshold on the forward transfer error |x2 - proj(H x1)| */
  double  confidence;        /* 0.995 */
  int32_t max_iters;         /* 2000 */
  int32_t seed;              /* of the counter-based sample generator */
  int32_t refine_iters;      /* 10: Levenberg-Marquardt steps after the DLT re-fit on the inliers; 0 returns the re-fit */
  int32_t _pad;
} vo_hom_params;

typedef struct {
  double  cost;              /* sum of squared forward transfer errors in pixels over the mask at the returned H */
  int32_t n_inliers;         /* consensus set of H0 */
  int32_t hypotheses;        /* four-point samples evaluated */
  int32_t best;              /* index of the winning sample */
  int32_t status;            /* 0, or VO_E_NUMERIC when no model with >= 4 inliers was found */
  int32_t lm_iters;          /* refinement steps tried */
  int32_t _pad;
} vo_hom_stats;

/* cv2.findFundamentalMat(p1, p2, cv2.FM_RANSAC, 3.0, 0.99): the two-view model that needs no intrinsics */
typedef struct {
  double  threshold;         /* 3.0 px: consensus threshold on the distance of a point to its epipolar line, in either view */
  double  confidence;        /* 0.99 */
  int32_t max_iters;         /* 1000 */
  int32_t seed;              /* of the counter-based sample generator */
  int32_t refit;             /* 0: F is the winning sample's model, as cv2 returns it; 1: the normalised eight-point re-fit on the inliers */
  int32_t _pad;
} vo_fund_params;

typedef struct {
  double  cost;              /* sum of err = max(d1^2, d2^2) in px^2 over the mask at the returned F */
  int32_t n_inliers;         /* consensus set of F0 */
  int32_t hypotheses;        /* seven-point samples evaluated */
  int32_t best;              /* index of the winning sample */
  int32_t status;            /* 0, or VO_E_NUMERIC when no model with >= 7 inliers was found */
  int32_t n_roots;           /* real roots (models) of the winning sample: 1 or 3 */
  int32_t models;            /* models scored over the whole search */
} vo_fund_stats;

/* Sim(3) / rigid alignment of two 3-D point sets, dst ~ s R src + t (vo_sim3_ransac, vo_sim3_fit): Umeyama's closed form inside the RANSAC
 * of cv2.estimateAffine3D(src, dst, ransacThreshold = 3.0, confidence = 0.99).  The six fields fill the 32 bytes: there is no padding */
typedef struct {
  double  threshold;         /* 3.0, in dst's units: consensus threshold on |dst - (s R src + t)| */
  double  confidence;        /* 0.99 */
  int32_t max_iters;         /* 1000 */
  int32_t seed;              /* of the counter-based sample generator */
  int32_t with_scale;        /* 1: a similarity (7 parameters); 0: s = 1, a rigid motion (Kabsch) */
  int32_t refit;             /* 1: Umeyama over the consensus set; 0: the winning sample's model is returned */
} vo_sim3_params;

typedef struct {
  double  cost;              /* sum of squared errors |dst - (s R src + t)|^2 over the mask at the returned model */
  int32_t n_inliers;         /* consensus set of the winning sample's model (vo_sim3_fit: rows fitted) */
  int32_t hypotheses;        /* three-point samples evaluated */
  int32_t best;              /* index of the winning sample (vo_sim3_fit: -1) */
  int32_t status;            /* 0, or VO_E_NUMERIC when no model with >= 3 inliers was found (vo_sim3_fit: fewer than 3 rows, or a degenerate set) */
  int32_t degenerate;        /* samples without a model: a coordinate that is not finite, collinear or coincident points, s <= 0 */
  int32_t refit;             /* 1: the returned model is Umeyama over the consensus set; 0: it is the winning sample's own */
} vo_sim3_stats;

/* cv2.decomposeHomographyMat(H, K) with cv2.filterHomographyDecompByVisibleRefpoints' two tests counted as votes, a ranking and an
 * ambiguity verdict (vo_homography_decompose, vo_homography_pose) */
typedef struct {
  double  ratio;             /* 0.75 (ORB-SLAM): a candidate is viable if n_good >= ratio x the largest n_good; in (0, 1] */
  double  threshold;         /* 1.0 px: Sampson threshold of the points outside the mask (divided by (fx + fy) / 2 internally) */
  double  hint[3];           /* plane-normal prior in view-1 camera coordinates (a ground plane: 0, 1, 0); read when use_hint != 0 */
  int32_t min_off;           /* 8: the best candidate is unambiguous once its n_off leads its rival's by this many points */
  int32_t use_hint;          /* 0 */
} vo_hpose_params;

typedef struct {
  double  sigma[3];          /* singular values of K^-1 H K divided by the middle one: s1 >= 1 >= s3; NaN without a solution */
  int32_t n_solutions;       /* 4; 1 for a rotation-only H (s1 - s3 <= 2^-26: t = n = 0); 0 without a solution */
  int32_t n_distinct;        /* 1, 2 or 4: entries that differ by 2^-20 or more in R, t or n (2: t || n, the two pairs coincide) */
  int32_t ambiguous;         /* 1: a distinct viable rival lies fewer than min_off behind the best in n_off and no hint was given */
  int32_t status;            /* 0, or VO_E_NUMERIC: det H = 0, a zero focal length or an entry that is not finite (a NaN H: no homography) */
  int32_t n_mask;            /* points with finite coordinates in the mask */
  int32_t n_good[4];         /* per ranked candidate: mask points in front of the plane in both views */
  int32_t n_off[4];          /* per ranked candidate: points outside the mask within the Sampson threshold of E = [t]x R */
  int32_t _pad;
} vo_hpose_stats;

/* the fields of cv2.KeyPoint that cv2.SIFT fills (the reference reads pt through cv2.KeyPoint_convert and hands the
 * objects back to compute(), src/extractor/extractor.py:114-122) */
typedef struct {
  float   x, y;              /* pt, pixels of the input image */
  float   size;              /* diameter of the meaningful neighbourhood */
  float   angle;             /* degrees, [0, 360) */
  float   response;          /* |contrast| of the refined extremum */
  int32_t octave;            /* packed: octave (low byte, signed), layer (second byte), sub-layer offset (third byte) */
} vo_sift_kp;

/* ---- context -------------------------------------------------------------------------------- */
int32_t vo_abi_version(void);
int32_t vo_device_count(int32_t* n);
/* width/height: image size; max_pts: capacity of the tracked point set (and of DLT batches);
 * max_level / win: pyramid depth and LK window the frame store is built for (3 / 31 in the
 * reference, extractor.py:16-19).  Levels stop early when the next one would be <= win in either
 * dimension, as cv2.buildOpticalFlowPyramid does. */
int32_t vo_ctx_create(int32_t device, int32_t width, int32_t height, int32_t max_pts,
                      int32_t max_level, int32_t win, vo_ctx** out);
/* BATCHED CONTEXT: `batch` independent sequences of identical shape advance in lockstep; every launch serves all of
 * them (the path is launch / latency bound per sequence, batching is what fills the 256 CUs).  With batch > 1 EVERY
 * array argument of every entry point below gains a leading dimension of length `batch` (images [batch][h][w],
 * points [batch][n][2], status [batch][n], X4 [batch][4][n], P0 [batch][12], K [batch][9], obs [batch][W][N][2],
 * out_pts [batch][max_corners][2], n_out [batch], stats [batch], ...); scalars (n, parameters) are shared.
 * vo_ctx_create(...) == vo_ctx_create_batched(..., 1, ...).
 * STREAMS: a context owns its streams (up to five: front end, side, bundle adjustment, copy-in, and a CU-masked form of the first in the gated
 * layout); the library is compiled with -fgpu-default-stream=per-thread, so its SYNCHRONOUS copies (uploads, read-backs, probes) run on the calling
 * thread's own default stream and never join the process's legacy null stream -- a caller that relies on null-stream ordering with its own HIP work
 * must synchronise explicitly (vo_sync). */
int32_t vo_ctx_create_batched(int32_t device, int32_t width, int32_t height, int32_t max_pts,
                              int32_t max_level, int32_t win, int32_t batch, vo_ctx** out);
int32_t vo_ctx_destroy(vo_ctx* ctx);
const char* vo_last_error(const vo_ctx* ctx);
int32_t vo_sync(vo_ctx* ctx);

/* ---- frames: pyramid + Scharr derivatives ---------------------------------------------------
 * Replaces the pyramid / derivative construction inside cv2.calcOpticalFlowPyrLK
 * (extractor.py:44-45,65-66 rebuild it on each of 4 calls per frame; here once per frame).
 * Pushing a frame rotates cur -> prev.  `stride` in bytes (>= width). */
int32_t vo_frame_push(vo_ctx* ctx, const uint8_t* img, int32_t stride);
/* Loader pre-filter (SURVEY.md 8f "next" row 2): cv2.bilateralFilter(img, d=5, sigmaColor=1.5, sigmaSpace=1.5) that
 * Loader.getImage applies to every frame (src/loader/loader.py:16-20,86), fused into the kernel that writes pyramid
 * level 0, so a raw frame can be pushed as read from disk.  d = 0: off (default; the drop-in classes receive frames the
 * reference's loader has already filtered); d < 0: diameter from sigma_space as OpenCV does; diameter <= 7.  A captured frame step
 * (vo_set_graph_mode) follows the setting: every accepted call gives the next step a new capture key. */
int32_t vo_set_prefilter(vo_ctx* ctx, int32_t d, double sigma_color, double sigma_space);
/* Lens undistortion of every frame entering the frame store: cv2.undistort(src, K, dist, None, newK) of OpenCV 4.4, i.e.
 * cv2.initUndistortRectifyMap (imgproc/undistort.cpp, no rectification, fixed-point map) followed by cv2.remap(INTER_LINEAR,
 * BORDER_CONSTANT 0) (imgproc/imgwarp.cpp).  The reference only ever loads rectified sets; this lets a raw-camera frame be pushed as it is.
 * Off by default.  On, every ingest path -- vo_frame_push, vo_frame_push_resident, vo_frame_step_resident / _host, vo_pipe_step /
 * _step_host -- runs kernel k_undistort in front of the level-0 kernel, so it precedes the bilateral pre-filter (vo_set_prefilter).
 * Definition (tests/undistort_model.py, bit for bit): per output pixel (j, i), in float64 without fused multiply-add,
 *   x = (j - cx') / fx', y = (i - cy') / fy', r2 = x x + y y, kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2)
 *   u = fx (x kr + p1 2xy + p2 (r2 + 2 x x)) + cx, v = fy (y kr + p1 (r2 + 2 y y) + p2 2xy) + cy
 * quantised to 1/32 pixel (rint, half to even): tap origin (sx, sy) = q >> 5, fractions q & 31; the four bilinear taps with the integer
 * weights (32 - fx5)(32 - fy5) 32, ... (sum 32768), a tap outside the image reads 0, dst = (sum + 16384) >> 15.  A map value that is not
 * finite, or a tap origin outside [-2, w] x [-2, h], gives 0.  OpenCV walks each map row with running sums over an inverted newK, so a live
 * cv2 can quantise a value within rounding noise of a tie differently: parity is with the model, as for use_harris.
 * K, newK: (fx, fy, cx, cy); newK == NULL: K.  dist: (k1, k2, p1, p2, k3, k4, k5, k6), the first n_dist of them, the rest 0.
 *   vo_set_undistort       builds the map on the host, waits for the context's streams and replaces the table.  VO_E_INVALID with nothing
 *                          changed: n_dist not one of 0, 4, 5, 8; dist == NULL with n_dist > 0; a value that is not finite; fx, fy, fx' or
 *                          fy' <= 0.  (VO_E_CAPACITY: an image side above 32766.)  Takes effect at the next enqueue; a captured frame step
 *                          is never replayed with another table.
 *   vo_clear_undistort     off again.
 *   vo_get_undistort       *on, and K [4], dist [8], newK [4] of the setting (zeros when off; any of the three may be NULL).
 *   vo_undistort           synchronous: `batch` images in (rows of `stride` bytes) and out (tight) with the current setting; the frame store
 *                          and its frame count are untouched.  VO_E_STATE: no setting is active.
 *   vo_undistort_map_read  the table the kernel reads: sxy [h][w][2] i16 (sx, sy), frac [h][w] u16 = fy5 * 32 + fx5, outside [h][w] u8
 *                          (any may be NULL).  VO_E_STATE: no setting is active. */
int32_t vo_set_undistort(vo_ctx* ctx, const double K[4], const double* dist, int32_t n_dist, const double* newK);
int32_t vo_clear_undistort(vo_ctx* ctx);
int32_t vo_get_undistort(vo_ctx* ctx, int32_t* on, double K[4], double dist[8], double newK[4]);
int32_t vo_undistort(vo_ctx* ctx, const uint8_t* img, int32_t stride, uint8_t* out);
int32_t vo_undistort_map_read(vo_ctx* ctx, int16_t* sxy, uint16_t* frac, uint8_t* outside);
/* Contrast-limited adaptive histogram equalisation of every frame entering the frame store: cv2.createCLAHE(clipLimit, tileGridSize)
 * .apply(img) of OpenCV 4.4 (imgproc/clahe.cpp, 8-bit path, histSize 256), the usual answer of a VO front end to exposure and shadow changes
 * that break the tracker's brightness constancy.  Not in the reference (its loaders do not equalise).  Off by default.  On, every ingest path
 * -- vo_frame_push, vo_frame_push_resident, vo_frame_step_resident / _host, vo_pipe_step / _step_host -- runs kernels k_clahe_lut and
 * k_clahe_apply in front of the level-0 kernel.  Order of the chain: undistortion (vo_set_undistort) -> CLAHE -> bilateral pre-filter
 * (vo_set_prefilter) or plain level 0 -> pyramid.
 * Definition (tests/clahe_model.py, bit for bit; a restatement -- no OpenCV source or binary was at hand, parity is with the model, as for
 * use_harris and vo_set_undistort):
 *   extension  w % tiles_x == 0 and h % tiles_y == 0: none.  Otherwise BOTH sides grow, by tiles_x - w % tiles_x columns and tiles_y - h % tiles_y
 *              rows (an axis that divides still grows by a whole tiles_*: 1241 x 376 at 8 x 8 becomes 1248 x 384), BORDER_REFLECT_101.
 *              tw = ext_w / tiles_x, th = ext_h / tiles_y, area = tw th.
 *   clip       clip_limit > 0: max((int)(clip_limit * area / 256), 1) (double, truncated); clip_limit == 0: no clipping.
 *   per tile   hist[256] over the tile of the extended image; clipped = sum of the excess above clip, bins cut; clipped / 256 added to every
 *              bin; residual = clipped % 256 != 0: step = max(256 / residual, 1), bins 0, step, 2 step .. (residual of them) get one more;
 *              lut[i] = clamp(rint((float)prefix_sum[i] * ((float)255 / (float)area)), 0, 255), rint = half to even.
 *   per pixel  (x, y) of the original image, value v, float32, no fused multiply-add: txf = (float)x * (1.0f / tw) - 0.5f, tx1 = floor(txf),
 *              xa = txf - tx1, xa1 = 1.0f - xa, then tx2 = min(tx1 + 1, tiles_x - 1), tx1 = max(tx1, 0); the same in y;
 *              dst = clamp(rint((lut[ty1][tx1][v] xa1 + lut[ty1][tx2][v] xa) ya1 + (lut[ty2][tx1][v] xa1 + lut[ty2][tx2][v] xa) ya), 0, 255).
 *   vo_set_clahe       (cv2.createCLAHE) waits for the context's streams, then replaces the setting.  VO_E_INVALID with nothing changed:
 *                      clip_limit negative or not finite; tiles_x or tiles_y outside 1 .. 16; an extension that is not smaller than the image
 *                      side on its axis (reflect-101 needs that).  Takes effect at the next enqueue; a captured frame step is never replayed
 *                      with another setting.
 *   vo_clear_clahe     off again.
 *   vo_get_clahe       *on and the setting (zeros when off; any of the three may be NULL).
 *   vo_clahe           (CLAHE::apply) synchronous: `batch` images in (rows of `stride` bytes) and out (tight) with the current setting; CLAHE
 *                      alone, NOT the undistortion in front of it; the frame store and its frame count are untouched.  VO_E_STATE: off.
 *   vo_clahe_lut_read  the tables the last launch (a frame entering the store, or vo_clahe) wrote: lut [batch][tiles_y][tiles_x][256] u8
 *                      (zeros before the first launch of a setting).  VO_E_STATE: off. */
int32_t vo_set_clahe(vo_ctx* ctx, double clip_limit, int32_t tiles_x, int32_t tiles_y);
int32_t vo_clear_clahe(vo_ctx* ctx);
int32_t vo_get_clahe(vo_ctx* ctx, int32_t* on, double* clip_limit, int32_t* tiles_x, int32_t* tiles_y);
int32_t vo_clahe(vo_ctx* ctx, const uint8_t* img, int32_t stride, uint8_t* out);
int32_t vo_clahe_lut_read(vo_ctx* ctx, uint8_t* lut);
/* frames preloaded into HBM (bench: inputs resident before the timed region); frames: [batch][n_frames][h][w] */
int32_t vo_seq_upload(vo_ctx* ctx, const uint8_t* frames, int32_t n_frames);
int32_t vo_frame_push_resident(vo_ctx* ctx, int32_t frame_index);           /* async */
/* parity probes: which = 0 prev / 1 cur; img_out (h_l x w_l u8), deriv_out (h_l x w_l x 2 i16), either may be NULL */
int32_t vo_pyramid_level_size(vo_ctx* ctx, int32_t level, int32_t* w, int32_t* h);
int32_t vo_pyramid_read(vo_ctx* ctx, int32_t which, int32_t level, uint8_t* img_out, int16_t* deriv_out);   /* sequence 0 */
int32_t vo_pyramid_read_seq(vo_ctx* ctx, int32_t seq, int32_t which, int32_t level, uint8_t* img_out, int16_t* deriv_out);

/* ---- KLT ------------------------------------------------------------------------------------
 * Replaces cv2.calcOpticalFlowPyrLK(prev, cur, p0, None, **lk_params) at extractor.py:44,65
 * (and, being deterministic, the redundant second call at :45,:66).
 * p0: n x 2 f32.  Outputs: p1 n x 2 f32, status n u8, err n f32, iters n x (max_level+1) i32
 * (iterations run per pyramid level, -1 = level skipped; may be NULL).
 * KEYPOINTS THAT ARE NOT HONEST NUMBERS (every tracker form: vo_klt_track*, vo_klt_track_resident, vo_tracks_track, vo_frame_step_*, vo_pipe_step*):
 *   OpenCV's cvFloor makes INT_MIN of a NaN and of every value outside [-2^31, 2^31), so such a p0 is outside the image on every level:
 *   status 0, err 0, every iters entry -1, and p1 is p0 passed through.  Here:
 *   - a p0 row with a component that is infinite or beyond int32 gives exactly that, p1 = p0 bit for bit (the scalings by 2^-l and 2 are exact);
 *   - a p0 row with a NaN component gives that status, err and iters, and a p1 row that is NOT FINITE.  Every entry that copies caller points
 *     to the device -- vo_klt_track, _fb, _init, _fb_init, vo_points_upload, vo_tracks_seed, vo_pipe_table_write(VO_PIPE_K_UV) -- stores such a
 *     row as (+inf, +inf); the synchronous calls hand the caller's own row back in p1 (and in p0r), the resident forms keep (+inf, +inf);
 *   - forward-backward: such a row has ok = 0 and an fb_err that is NaN or +inf, below no threshold;
 *   - the row draws no exclusion disc (vo_shi_tomasi below) and fails the keep rule of a track table or of the closed loop.
 *   Nothing on the device turns a finite point into a NaN one (front-end contract).  Guesses keep their own rule (below). */
int32_t vo_klt_default_params(vo_klt_params* p);
int32_t vo_klt_track(vo_ctx* ctx, const float* p0, int32_t n, const vo_klt_params* prm,
                     float* p1, uint8_t* status, float* err, int32_t* iters);
/* resident form: the point set lives in HBM and is advanced in place (p <- tracked p) */
int32_t vo_points_upload(vo_ctx* ctx, const float* p, int32_t n);
/* iters (may be NULL): n x (max_level+1) of the last resident track, as in vo_klt_track */
int32_t vo_points_download(vo_ctx* ctx, float* p, uint8_t* status, float* err, int32_t* iters, int32_t n);
int32_t vo_klt_track_resident(vo_ctx* ctx, int32_t n, const vo_klt_params* prm);  /* async */

/* ---- forward-backward check ------------------------------------------------------------------
 * What max_bidir_error of extend_tracks / extend_landmarks (extractor.py:44-47,65-68) means once the image order of the second call is
 * fixed as in the OpenCV sample it copies (notebooks/tracking.py:39-42; the reference tracks forward twice):
 *   p1, st, err = LK(prev, cur, p0)    unchanged, bit for bit vo_klt_track
 *   p0r         = LK(cur, prev, p1)    template from the CURRENT frame (image + Scharr), target the previous frame
 *   fb_err      = max(|p0 - p0r|) over x, y (f32)        ok = fb_err < max_err (max_err rounded to f32 once; NaN fails)
 * One launch (k_klt_track_fb, one wave per keypoint) runs both passes.
 *   vo_klt_track_fb   the synchronous form: vo_klt_track's arguments and layout ([batch][n]) plus p0r [batch][n][2], fb_err [batch][n] f32
 *   vo_set_fb_check   per context; +inf (the default) = off, NaN -> VO_E_INVALID.  Takes effect at the next enqueue.  A finite threshold
 *                     makes vo_tracks_track and the TRACK stage of vo_pipe_step / vo_pipe_step_host track with the check and AND `ok`
 *                     into their keep rule: a point that fails it dies exactly like one outside the image (extractor.py:49-53,74-78).
 *                     Off, they run the plain tracker as before.  vo_klt_track_resident and the fused vo_frame_step_* never check.
 *   vo_fb_read        synchronous, no step in flight (else VO_E_STATE): ok [batch][n] u8 and fb_err [batch][n] f32 (either may be NULL)
 *                     of the dense point set of the last track, if it ran with the check (else VO_E_STATE) -- list order of the track
 *                     table, [landmarks | candidates] in the closed loop; dead slots read ok = 0, fb_err = NaN. */
int32_t vo_klt_track_fb(vo_ctx* ctx, const float* p0, int32_t n, const vo_klt_params* prm, float* p1, uint8_t* status, float* err,
                        float* p0r, float* fb_err, int32_t* iters);
int32_t vo_set_fb_check(vo_ctx* ctx, float max_err);
int32_t vo_get_fb_check(vo_ctx* ctx, float* max_err);
int32_t vo_fb_read(vo_ctx* ctx, uint8_t* ok, float* fb_err, int32_t n);

/* ---- motion-predicted initial flow -----------------------------------------------------------
 * The reference only ever calls cv2.calcOpticalFlowPyrLK with flags = 0 (extractor.py:44,65): every point starts at its previous position.
 * This is OpenCV's other documented mode, OPTFLOW_USE_INITIAL_FLOW (video/lkpyramid.cpp): the caller hands a guess g per point, and with
 * `top` the highest pyramid level actually used (after truncation)
 *   at level == top:   nextPt = g * (float)(1.0 / (1 << top))    per component, f32
 *   everything else as vo_klt_track: the template is taken at p0 / 2^level in the previous frame; the propagation to the lower levels, the
 *   out-of-range and min-eigenvalue skips (a skipped top level hands the scaled guess down as it hands prevPt down), the exits, status,
 *   err and iters are unchanged.
 *   A guess with a component that is not finite (OpenCV leaves that undefined): the point starts from p0.
 *   g == p0 gives the unseeded tracker's bits: the same f32 expression on the same value.
 * Kernels k_klt_seeded / k_klt_seeded_fb (one wave per keypoint; the forward pass is seeded, the backward pass LK(cur, prev, p1) is not).
 *   vo_klt_track_init      vo_klt_track with guess [batch][n][2] f32; synchronous, the same layouts.  guess == NULL: exactly vo_klt_track.
 *   vo_klt_track_fb_init   vo_klt_track_fb likewise.
 *   vo_set_klt_predict     per context: VO_KLT_PREDICT_OFF (0, the default) or VO_KLT_PREDICT_CONST_VELOCITY (1); anything else ->
 *                          VO_E_INVALID.  Takes effect at the next enqueue.  On, vo_tracks_track and the TRACK stage of vo_pipe_step /
 *                          vo_pipe_step_host write a guess per point of the tracked set on the device and run the seeded kernel (with a
 *                          finite vo_set_fb_check threshold the seeded forward-backward kernel).  The predictor, f32 per component:
 *                              g = uv + (uv - prev);   prev missing or not finite: g = uv;   no clamping -- a guess outside the image
 *                              meets the tracker's own out-of-range rules
 *                          uv = the point the tracker starts from; prev = the track's position one frame earlier: the track table's ring
 *                          entry of frame t - 2 (missing for a track born at t - 1), the closed loop's history entry hist_len - 2 of the
 *                          keypoint row behind the entry (LM_K[i] for a landmark, CAND[i - n_landmarks] for a candidate; missing when
 *                          hist_len < 2).  vo_klt_track_resident and the fused vo_frame_step_* never predict: they have no history.
 *   vo_klt_guess_read      synchronous, no step in flight (else VO_E_STATE): guess [batch][n][2] f32, what the last track started from,
 *                          if a predictor ran for it (else VO_E_STATE) -- the tracker's point order; dead slots read NaN. */
enum { VO_KLT_PREDICT_OFF = 0, VO_KLT_PREDICT_CONST_VELOCITY = 1 };
int32_t vo_klt_track_init(vo_ctx* ctx, const float* p0, const float* guess, int32_t n, const vo_klt_params* prm,
                          float* p1, uint8_t* status, float* err, int32_t* iters);
int32_t vo_klt_track_fb_init(vo_ctx* ctx, const float* p0, const float* guess, int32_t n, const vo_klt_params* prm, float* p1, uint8_t* status,
                             float* err, float* p0r, float* fb_err, int32_t* iters);
int32_t vo_set_klt_predict(vo_ctx* ctx, int32_t mode);
int32_t vo_get_klt_predict(vo_ctx* ctx, int32_t* mode);
int32_t vo_klt_guess_read(vo_ctx* ctx, float* guess, int32_t n);

/* ---- Shi-Tomasi re-detection ----------------------------------------------------------------
 * Replaces the exclusion-mask loop + cv2.goodFeaturesToTrack(img, mask=mask, **shitomasi_params)
 * at extractor.py:103-112 on the CURRENT frame.  cur_pts (n_cur x 2 f32, may be NULL) are the
 * tracked keypoints; discs of `mask_radius` at int32-truncated coordinates are excluded
 * (cv2.circle fill semantics).  `mask` (h x w u8, may be NULL) is an optional explicit mask that
 * is AND-ed with the discs.  out_pts: max_corners x 2 f32 (integer-valued x, y); *n_out set.
 * A centre with a component that is NaN or outside [-2^31, 2^31) draws nothing, on every path that draws discs (vo_shi_tomasi*,
 * vo_tracks_detect, vo_frame_step_*, the closed loop): np.int32() makes INT_MIN of it and cv2.circle clips that away.  Any other centre,
 * however far outside the image, is clipped row by row.
 * The detector is a choice of RESPONSE MAP (vo_st_params): the minimum eigenvalue (default), the Harris response (use_harris), or the
 * FAST-9/16 corner score of cv2.FastFeatureDetector (fast_threshold = 1..254; k_fast_score, csrc/vo_fast.hip -- the detector ORB builds
 * on; orientation and descriptor: vo_brief_* below).  What follows the map is the same for all three on every path that takes a vo_st_params
 * (vo_shi_tomasi*, vo_tracks_detect, vo_frame_step_*, vo_pipe_params.st): quality threshold against the masked maximum, 3 x 3 >= test,
 * mask, rank order (value, then pixel index, both descending), min-distance grid, max_corners.  With the FAST response the map that
 * vo_shi_tomasi_read returns is the score map (0 where no corner, also within 3 pixels of a border), and the resident forms keep it and
 * the mask.  A fast_threshold outside 0..254, or one > 0 together with use_harris, is VO_E_INVALID on each of those paths (vo_pipe_create
 * for the closed loop) with nothing enqueued.  Contexts are at least 7 x 7 pixels: the smallest frame that holds a whole FAST ring. */
int32_t vo_st_default_params(vo_st_params* p);
int32_t vo_shi_tomasi(vo_ctx* ctx, const float* cur_pts, int32_t n_cur, int32_t mask_radius,
                      const uint8_t* mask, const vo_st_params* prm, float* out_pts, int32_t* n_out);
int32_t vo_shi_tomasi_resident(vo_ctx* ctx, int32_t n_cur, int32_t mask_radius,
                               const vo_st_params* prm);                      /* async; uses the resident points */
int32_t vo_shi_tomasi_fetch(vo_ctx* ctx, float* out_pts, int32_t* n_out);     /* sync + copy out */
/* Parameter rules, the same on every path that takes a vo_st_params (OpenCV asserts them): quality_level > 0 (NaN, 0 and -0.0 are refused),
 * min_distance >= 0 (NaN and negatives are refused; any finite value and +inf are accepted -- a distance beyond the image diagonal yields
 * exactly one corner, the strongest candidate), max_corners >= 0 (0 = all, at most 4096).  A refused call is VO_E_INVALID with nothing
 * enqueued.  min_distance < 1 applies no distance rule; a fractional one is taken as it is (dx^2 + dy^2 < min_distance^2 in double).
 * vo_shi_tomasi_resident_limit: vo_shi_tomasi_resident with a corner limit per sequence, limits [batch] on the host (copied before the call
 * returns).  Sequence b ends with the first min(max(limits[b], 0), max_corners) corners of the unlimited call, in the same order, and n_out
 * says so.  It is the closed loop's detection (the limit read on the device, the candidate list consumed in short rank-ordered chunks) as a
 * call of its own; vo_tuning.st_host_limit makes it ignore the limits. */
int32_t vo_shi_tomasi_resident_limit(vo_ctx* ctx, int32_t n_cur, int32_t mask_radius, const vo_st_params* prm, const int32_t* limits);
/* parity probes: min-eigenvalue map (h x w f32) and the mask actually used (h x w u8) of the last SYNCHRONOUS call
 * (vo_shi_tomasi).  The resident forms keep neither -- the map never leaves the kernel that forms it and the mask is handed
 * back clean for the next frame -- and eig_out / mask_out then return VO_E_STATE (vo_tuning.st_keep_eig makes the
 * resident forms keep them); n_candidates (local maxima above the quality threshold) is always available.
 * More than 16384 candidates are consumed in rank-ordered chunks, like OpenCV's scan; VO_E_CAPACITY only beyond 262144. */
int32_t vo_shi_tomasi_read(vo_ctx* ctx, float* eig_out, uint8_t* mask_out, int32_t* n_candidates);

/* ---- sub-pixel corner refinement --------------------------------------------------------------
 * The reference keeps the integer corners of cv2.goodFeaturesToTrack (extractor.py:111).  This is the call OpenCV's own pipelines put right
 * behind it, cv2.cornerSubPix (imgproc/cornersubpix.cpp with getRectSubPix 8u -> 32f): per corner, iterate
 *   S    = (2 win_y + 3) x (2 win_x + 3) bilinear samples (f32) of level 0 around the corner, pixel coordinates clamped to the image
 *   sums = over the window, weighted by a separable exp(-t^2) mask (zero inside the zero zone): gxx, gxy, gyy, gxx*px + gxy*py,
 *          gxy*px + gyy*py of the central differences of S, in float64, in a fixed order (tests/subpix_model.py states it)
 *   step = corner + (2 x 2 solve), rounded to f32; stop when the system is singular (|det| <= DBL_EPSILON^2), the corner leaves
 *          [0, w) x [0, h), max_count steps were taken, or a step is no longer than epsilon
 * and a result further than win from the input on either axis goes back to the input.  A result just outside the image is possible (the step
 * that left it is kept when within win), as in OpenCV; the tracker's and the keep rule's range tests meet it in the next frame.  A corner that
 * is not finite or lies outside [0, w) x [0, h) comes back unchanged (OpenCV asserts there; NaN rows pad a batch).
 * Parameters: win_x, win_y half sizes in 1..7; zero_x, zero_y half sizes of the zero zone, -1 = none; max_count clamped to 1..100;
 * epsilon clamped at 0.  Defaults: (5, 5), (-1, -1), 40, 0.001.
 * Kernel k_corner_subpix: one wave per corner; parity with OpenCV itself is not pinned, the numpy model is the definition (bit for bit).
 *   vo_corner_subpix   synchronous.  which = 0 the previous / 1 the current frame of the frame store; corners, out [batch][n][2] f32;
 *                      iters [batch][n] i32 (steps counted) and flags [batch][n] u8 may be NULL.  flags: 0 ran to a stopping test,
 *                      1 singular, 2 left the image, 3 reverted to the input, 4 input not usable.
 *                      VO_E_INVALID, nothing enqueued: win outside 1..7, an image smaller than 2 * win + 5 on either axis, a NaN epsilon,
 *                      n > max_pts.  VO_E_STATE: the named frame has not been pushed.
 *   vo_set_subpix      per context; NULL = off (the default); the same parameter checks.  Takes effect at the next enqueue.  On,
 *                      vo_tracks_detect and the DETECT stage of vo_pipe_step / vo_pipe_step_host enqueue the kernel on the detection's stream
 *                      between the Shi-Tomasi selection and the spawn: the corner rows are refined in place against the current frame, and the
 *                      new tracks / candidates (uv, uv_first, history entry 0) are born at the refined positions.  The min-distance rule is not
 *                      run again (OpenCV does not either).  Results do not depend on the stream layout.
 *                      These never refine: vo_shi_tomasi; vo_shi_tomasi_resident / vo_shi_tomasi_fetch when not behind a vo_tracks_detect
 *                      (after one, vo_shi_tomasi_fetch returns the refined rows); the fused vo_frame_step_*.
 *   vo_subpix_read     synchronous, no step in flight (else VO_E_STATE): the integer corners raw [batch][n][2] f32, iters, flags (any may be
 *                      NULL) of the last vo_tracks_detect / DETECT stage, if it refined (else VO_E_STATE; a vo_corner_subpix call in between
 *                      also ends it).  Slots beyond a sequence's corner count read raw = NaN, iters 0, flags 4. */
typedef struct { int32_t win_x, win_y, zero_x, zero_y, max_count, _pad; double epsilon; } vo_subpix_params;  /* 32 bytes */
int32_t vo_subpix_default_params(vo_subpix_params* p);
int32_t vo_corner_subpix(vo_ctx* ctx, int32_t which, const float* corners, int32_t n, const vo_subpix_params* prm, float* out, int32_t* iters,
                         uint8_t* flags);
int32_t vo_set_subpix(vo_ctx* ctx, const vo_subpix_params* prm);
int32_t vo_get_subpix(vo_ctx* ctx, int32_t* on, vo_subpix_params* prm);
int32_t vo_subpix_read(vo_ctx* ctx, float* raw, int32_t* iters, uint8_t* flags, int32_t n);

/* ---- oriented BRIEF descriptor (the descriptor half of ORB) ------------------------------------
 * The reference's Extractor names it: cv2.ORB_create() (src/extractor/extractor.py:30-31), extract(..., describe=True) for any detector
 * (:119-122), and the commented "Alternative Method" of Pipeline.step (src/pipeline/pipeline.py:105-121), which matches landmarks to
 * re-detected keypoints by descriptor.  The detector half is the FAST response above; this is orientation by intensity centroid and a steered
 * 256-bit BRIEF at the detected corners.  Neither OpenCV nor its learned sampling table is part of this project: parity with cv2.ORB is not
 * pinned, the numpy model tests/brief_model.py is the definition (bit for bit), and the sampling pattern is the caller's table -- a user who has
 * OpenCV uploads ORB's own.  Per corner, at the integer pixel (x, y) = (rint(cx), rint(cy)) (half to even) of level 0 of the named frame
 * (behind undistortion, CLAHE and the pre-filter where those are on):
 *   margin   M = 24 (21 for the furthest rotated sample + 3 for the blur).  Described iff M <= x <= w-1-M and M <= y <= h-1-M; any other corner:
 *            flags = 1, 32 zero bytes, angle 0.  A row that is not finite: flags = 2, the same zeros.  No border is ever extrapolated.
 *   angle    ORB's IC_Angle on the raw (un-blurred) image: m10 = sum u I(x+u, y+v), m01 = sum v I(x+u, y+v) over |v| <= 15, |u| <= umax[|v|],
 *            umax = {15,15,15,15,14,14,14,13,13,12,11,10,9,8,6,3}; exact in int32.  Both 0: c = 1, s = 0, angle = 0.  Otherwise in float64
 *            r = sqrt(m10*m10 + m01*m01), c = (f32)(m10 / r), s = (f32)(m01 / r); angle = atan2(m01, m10) in degrees in [0, 360) as f32.
 *            The angle is reported only and never enters the descriptor (ORB goes through fastAtan2 and cos / sin; this keeps the bits exact).
 *   blur     separable 7-tap integer Gaussian (sigma ~ 2) g = {18,33,49,56,49,33,18}, sum 256: horizontal sums (they fit u16), the vertical
 *            pass over those, S = (v + 32768) >> 16.  ORB's GaussianBlur(7 x 7, 2) in spirit, not bit for bit.
 *   tests    the pattern: 256 rows (x1, y1, x2, y2) int8, every coordinate in [-15, 15], a row's two points differ.  Per point in float32
 *            without contraction fx = x1*c - y1*s, fy = x1*s + y1*c (two rounded products, one rounded sum), ix = rint(fx), iy = rint(fy) half
 *            to even.  Bit i = S(x+ix1, y+iy1) < S(x+ix2, y+iy2), in byte i / 8 at bit i % 8 (LSB first).
 *   default  pattern: BRIEF's isotropic Gaussian sampling, N(0, 6^2) rounded, defined by tools/gen_brief_pattern.py (csrc/vo_brief_pattern.h).
 * Not ORB by itself: the corners are single-scale.  The 8-level pyramid, the Harris re-ranking and the per-level quotas are vo_orb_detect_compute's
 * (section "multi-scale ORB features"), which describes with this same code; the learned table and fastAtan2 are in neither.
 * Kernel k_brief_describe (csrc/vo_brief.hip): one wave per corner, the 49 x 49 tile and its blur in LDS.
 *   vo_brief_default_pattern  out[1024]: the default table; needs no context.
 *   vo_brief_params           n_bits must be 256; the rest is room to grow and must be 0.  vo_brief_default_params fills it.
 *   vo_brief_compute          synchronous.  which = 0 the previous / 1 the current frame of the frame store; corners [batch][n][2] f32; prm NULL =
 *                             the defaults; pattern NULL = the default table; desc [batch][n][32] u8; angle [batch][n] f32 and flags [batch][n] u8 may
 *                             be NULL.  VO_E_INVALID, nothing enqueued: n > max_pts, n_bits != 256, a pattern coordinate outside +-15, a pattern row
 *                             with equal points.  VO_E_STATE: the named frame has not been pushed.  A context smaller than 49 pixels on either axis
 *                             is legal: every corner comes back with flags = 1.
 *   vo_set_brief              per context; prm NULL = off (the default); pattern NULL = the default table; the same checks.  Takes effect at the next
 *                             enqueue (a launch takes the table by value: steps in flight keep theirs).  On, vo_tracks_detect and the DETECT stage of
 *                             vo_pipe_step / vo_pipe_step_host enqueue the kernel on the detection's stream behind the selection and BEFORE the
 *                             sub-pixel refinement of vo_set_subpix, so it always sees the integer corners.  The descriptors live in a side buffer:
 *                             no table, record or index list of the track table or the closed loop changes by a bit, on any stream layout.
 *                             These never describe: vo_shi_tomasi*, outside a vo_tracks_detect; the fused vo_frame_step_* (so no captured graph
 *                             holds the kernel).
 *   vo_get_brief              *on = 0 / 1; prm (may be NULL) = the setting, the defaults when off.  vo_brief_pattern_read: the table in effect.
 *   vo_brief_read             synchronous, no step in flight (else VO_E_STATE): desc [batch][n][32], angle, flags (any may be NULL) of the last
 *                             vo_tracks_detect / DETECT stage in corner order, if it described (else VO_E_STATE; a vo_brief_compute call in between
 *                             also ends it).  Slots beyond a sequence's corner count read zeros with flags = 2. */
typedef struct { int32_t n_bits /* 256 */, _pad; int32_t reserved[6]; } vo_brief_params;  /* 32 bytes */
int32_t vo_brief_default_pattern(int8_t* out);
int32_t vo_brief_default_params(vo_brief_params* p);
int32_t vo_brief_compute(vo_ctx* ctx, int32_t which, const float* corners, int32_t n, const vo_brief_params* prm, const int8_t* pattern,
                         uint8_t* desc, float* angle, uint8_t* flags);
int32_t vo_set_brief(vo_ctx* ctx, const vo_brief_params* prm, const int8_t* pattern);
int32_t vo_get_brief(vo_ctx* ctx, int32_t* on, vo_brief_params* prm);
int32_t vo_brief_pattern_read(vo_ctx* ctx, int8_t* out);
int32_t vo_brief_read(vo_ctx* ctx, uint8_t* desc, float* angle, uint8_t* flags, int32_t n);

/* ---- DLT triangulation ----------------------------------------------------------------------
 * Replaces cv2.triangulatePoints(P0, P1, uv0, uv1) at extractor.py:270 and the reprojection
 * statistics TriangulatorNL.refine filters on (src/extractor/triangulate.py:87-111,139).
 * P0, P1: 3x4 f32 row-major (already rounded to f32 as extractor.py:268-269 does);
 * uv0, uv1: n x 2 f32.  X4: 4 x n f32 (OpenCV layout, homogeneous, unit norm).
 * Optional filter statistics (computed in f64 on the f32-rounded, dehomogenised point exactly as
 * the reference does): K 3x3 f64, H0/H1 4x4 f64 row-major -> depth1 n f64 ((H1 [X;1])_z) and
 * reproj n f64 ((|e0| + |e1|) / 2).  Pass K = NULL to skip them. */
int32_t vo_triangulate_dlt(vo_ctx* ctx, const float* P0, const float* P1, const float* uv0,
                           const float* uv1, int32_t n, float* X4,
                           const double* K, const double* H0, const double* H1,
                           double* depth1, double* reproj);

/* resident form for the bench (inputs uploaded once, kernel enqueued per frame, results fetched at the frame's end) */
int32_t vo_dlt_upload(vo_ctx* ctx, const float* P0, const float* P1, const float* uv0, const float* uv1,
                      int32_t n, const double* K, const double* H0, const double* H1);
int32_t vo_dlt_resident(vo_ctx* ctx);                                          /* async */
int32_t vo_dlt_fetch(vo_ctx* ctx, float* X4, double* depth1, double* reproj);

/* ---- sliding-window bundle adjustment -------------------------------------------------------
 * Replaces the scipy.optimize.least_squares call in BundleAdjuster.adjust
 * (src/bundle_adjuster/bundle_adjuster.py:189-194) and its objective (:18-65).
 * Problem layout (float64, C-contiguous):
 *   K       3x3
 *   poses   W x 6   (rvec, tvec) world->camera; slot 0 = newest frame (as :169-176)
 *   points  N x 3
 *   obs     W x N x 2 pixel observations; NaN in obs[i][j][0] = landmark j not seen in slot i
 * Same cost as the reference (Huber on the per-observation pixel-error norm, f_scale 1, no gauge
 * fixing); solver = analytic Jacobian, IRLS-weighted J^T J, landmark Schur complement (f64 MFMA
 * SYRK), dense Cholesky, Levenberg-Marquardt -- see DESIGN.md. */
int32_t vo_ba_default_params(vo_ba_params* p);
int32_t vo_ba_adjust(vo_ctx* ctx, const double* K, const double* poses, const double* points,
                     const double* obs, int32_t n_slots, int32_t n_pts, const vo_ba_params* prm,
                     double* poses_out, double* points_out, vo_ba_stats* stats);
/* resident form for the bench: upload once, solve repeatedly from the same x0 */
int32_t vo_ba_upload(vo_ctx* ctx, const double* K, const double* poses, const double* points,
                     const double* obs, int32_t n_slots, int32_t n_pts);
int32_t vo_ba_solve_resident(vo_ctx* ctx, const vo_ba_params* prm);          /* async */
/* a BANK of n_problems resident problems of one shape, one selected per solve (host-side pointer switch, nothing enqueued): a sliding
 * window never presents the same problem twice, so the bench's sequences cycle through distinct problems without an upload in the loop.
 * poses [n_problems][batch][W][6], points [n_problems][batch][N][3], obs [n_problems][batch][W][N][2]; K [batch][9] */
int32_t vo_ba_upload_bank(vo_ctx* ctx, const double* K, const double* poses, const double* points, const double* obs,
                          int32_t n_slots, int32_t n_pts, int32_t n_problems);
int32_t vo_ba_select_problem(vo_ctx* ctx, int32_t k);
int32_t vo_ba_fetch(vo_ctx* ctx, double* poses_out, double* points_out, vo_ba_stats* stats);
/* parity probes at the uploaded x0 (no iteration):
 *   residual: m f64 in the reference's order (slot-major, ascending landmark; :18-65)
 *   normal equations with Huber IRLS weights: Hpp W x 6 x 6, gp W x 6, Hll N x 3 x 3, gl N x 3,
 *   reduced camera system at damping lambda: S 6W x 6W, rhs 6W; one LM step dposes W x 6, dpoints N x 3.
 *   Any output pointer may be NULL. */
int32_t vo_ba_probe(vo_ctx* ctx, double lambda, double huber_delta, double* residual, int32_t* n_obs,
                    double* cost, double* Hpp, double* gp, double* Hll, double* gl, double* S,
                    double* rhs, double* dposes, double* dpoints);
/* the same probe with the weights and cost of any loss (VO_LOSS_*, f_scale = C); vo_ba_probe is its VO_LOSS_HUBER case.
 * An unknown loss, an f_scale <= 0 / NaN, or a robust loss's f_scale outside [VO_BA_F_SCALE_MIN, VO_BA_F_SCALE_MAX]: VO_E_INVALID, nothing enqueued. */
int32_t vo_ba_probe_loss(vo_ctx* ctx, double lambda, int32_t loss, double f_scale, double* residual, int32_t* n_obs,
                         double* cost, double* Hpp, double* gp, double* Hll, double* gl, double* S,
                         double* rhs, double* dposes, double* dpoints);

/* ---- landmark-sharded bundle adjustment of ONE problem (BASELINE config 5) -------
 * The reference has no multi-device path (single Python process, src/pipeline/pipeline.py:155-156 calls adjust once
 * per frame); this is the exchange step north_star names ("RCCL over xGMI only for the shared-landmark BA
 * reduction").  The landmarks of one window are dealt round-robin to S = n_ranks x batch shards: shard s = rank *
 * batch + b owns landmarks j with j % S == s together with ALL their observations; the W poses are replicated.
 * Every shard eliminates its own landmarks; the shared quantity is the reduced camera system every landmark
 * contributes to.  Per LM iteration: ONE in-place RCCL all-reduce (sum, f64) of the packed
 * [Gram tiles of Y^ (E and r) | camera sums H_pp, g_p, cost | per-rank max|g_l| slots] (23 KB at W = 10, 78 KB at
 * W = 20) and one of the 4 step statistics; every rank then solves the 6W x 6W system redundantly and takes the
 * same accept/reject decision.  The batch dimension of a batched context acts as `batch` shards on one GPU (summed
 * by a kernel) -- useful on its own for tests and for filling one GPU with a single large problem.
 *   vo_comm_unique_id: 128-byte RCCL id made by rank 0; distribute it to the other ranks by any means.
 *   vo_comm_init:      one communicator per context (one process per GPU); n_ranks = 1 is valid.
 *   vo_ba_set_sharded: on = 1: the `batch` problems of vo_ba_upload / vo_ba_adjust are shards of one problem
 *                      (same K and poses in every entry, shard-local points / obs, all shards padded to the same
 *                      N with unobserved landmarks at the origin).
 *   vo_ba_gather_points: points of every shard of every rank after a solve, [n_ranks][batch][N][3]. */
#define VO_COMM_ID_BYTES 128
#define VO_COMM_MAX_RANKS 16
int32_t vo_comm_unique_id(uint8_t* id_out /* VO_COMM_ID_BYTES */);
int32_t vo_comm_init(vo_ctx* ctx, int32_t n_ranks, int32_t rank, const uint8_t* id);
int32_t vo_comm_destroy(vo_ctx* ctx);
int32_t vo_ba_set_sharded(vo_ctx* ctx, int32_t on);
int32_t vo_ba_gather_points(vo_ctx* ctx, double* points_all);

/* ---- 3D-2D pose (SURVEY.md 8f "next" row 1) ---------------------------------------------------
 * Replaces cv2.solvePnPRansac(pts3d, pts2d, K, None, reprojectionError, iterationsCount, confidence) in
 * Extractor.camera_pose(corr='3D-2D') (src/extractor/extractor.py:174-191): RANSAC over P3P hypotheses (one wave per
 * hypothesis, 256 per batch and sequence, iteration bound updated like OpenCV's RANSACUpdateNumIters), consensus set
 * = squared reprojection error <= reproj_err^2, Gauss-Newton refinement of (rvec, tvec) over the consensus set.
 * OpenCV's sample sequence cannot be reproduced (own RNG, EPnP on 5 points): parity is statistical -- same consensus
 * set and minimiser whenever the inlier set is unambiguous; the algorithm itself is defined by oracle/pnp_oracle.py.
 * K [batch][9]; pts3d [batch][n][3], pts2d [batch][n][2] f32 (NaN rows are never inliers);
 * rvec, tvec [batch][3] f64 (x_cam = R(rvec) X + tvec); inlier_mask [batch][n] u8 (may be NULL); stats [batch].
 * Held to an independent float64 model (tests/pnp_model.py; test_pnp_model.py on the CPU, test_gpu_pnp_model.py on the kernel):
 *   P3P accuracy    every solution of Grunert's quartic is polished by Newton on the three distance equations in the depths (at most 16
 *                   steps, skipped where the squared sides are already met to 1e-10 of the squared smallest altitude).  A returned pose
 *                   reprojects the three points it was solved from within 2e-8 px (measured over 7 x 400 sets: general, wall, far, 5 cm
 *                   triangles, near-equilateral, isosceles, near-collinear; bound 1e-6 px).  The quartic alone was off by up to 74 px on
 *                   a wall and 7 px on tiny and symmetric triangles.  A double root that rounding split into a complex pair is kept, and where
 *                   2 (cos gamma - v cos alpha) is under 1e-3 the depth ratio u is also taken from its quadratic (two solutions share v).
 *   missed roots    a triangle of under a pixel (three points within 5 cm at 10-40 m) leaves the quartic's coefficients four or five
 *                   digits: 23 of 400 such sets lose their roots (22 yield no pose at all).  One of 400 near-equilateral sets (1 mm off
 *                   the symmetry) still loses one near-double root; next to a double root (one float32 near-collinear set, conditioning of the
 *                   three reprojections 0.016 px per unit pose) Newton from either quartic root lands on the same neighbour.
 *   consensus       no cheirality test: a point behind the camera that reprojects within reproj_err counts, as with
 *                   cv2.projectPoints; NaN rows and points with p2 == 0 never count.  The division is v_rcp_f64 + two Newton steps:
 *                   a point whose squared error is within 8 x 2^-52 x (e (|u| + |v|) + e^2) of reproj_err^2 may fall on either side.
 *   rvec            within 1e-2 of pi the angle comes from atan2 (|w| / 2, c) and the axis from the symmetric part of R (a few 2^-52);
 *                   th / (2 sin th) with th = acos(c) was off by 6e-6 rad at pi - 1e-5 and 2e-4 rad at pi - 2e-6. */
int32_t vo_pnp_default_params(vo_pnp_params* p);
int32_t vo_pnp_ransac(vo_ctx* ctx, const double* K, const float* pts3d, const float* pts2d, int32_t n,
                      const vo_pnp_params* prm, double* rvec, double* tvec, uint8_t* inlier_mask, vo_pnp_stats* stats);
/* resident form: correspondences uploaded once, a solve enqueued per frame with no host synchronisation (`blind_batches`
 * batches of 32, then 256 hypotheses each, early-exiting once the iteration bound is reached: 2 cover down to ~42 % inliers), results
 * fetched later; a sequence whose bound was not reached reports status VO_E_CAPACITY (pose = best so far). */
int32_t vo_pnp_upload(vo_ctx* ctx, const double* K, const float* pts3d, const float* pts2d, int32_t n);
int32_t vo_pnp_solve_resident(vo_ctx* ctx, const vo_pnp_params* prm, int32_t blind_batches);        /* async */
int32_t vo_pnp_fetch(vo_ctx* ctx, double* rvec, double* tvec, uint8_t* inlier_mask, vo_pnp_stats* stats);

/* ---- 2D-2D bootstrap pose (SURVEY.md 8f "next" row 4, pose part) ---------------------------------
 * Replaces cv2.findEssentialMat(..., method=RANSAC) + cv2.recoverPose in Extractor.camera_pose(corr='2D-2D')
 * (src/extractor/extractor.py:162-172; Pipeline._get_init_state, src/pipeline/pipeline.py:63): RANSAC over Nister
 * five-point essential matrices (a lane per sample, <= 10 models each, a wave per model for the consensus count),
 * consensus = squared Sampson distance <= (threshold / mean focal length)^2, iteration bound as RANSACUpdateNumIters
 * with 5 model points; the best model is returned as found (OpenCV does not re-fit); then the four (R, t)
 * candidates of E and OpenCV's cheirality vote by DLT triangulation of the inliers.  Sample draws differ from
 * OpenCV's: statistical parity; the algorithm is defined by oracle/essential_oracle.py.
 * Every root of the 10th-degree determinant is refined by up to 12 Gauss-Newton steps on the ten cubic constraints (in the
 * unit 4-vector of null-space coordinates), since the determinant alone loses up to half the digits of a root.  Measured
 * against an independent float64 model (tests/essential_model.py) on general, forward, sideways, rotating, planar,
 * fronto-parallel and wide-angle five-point sets (32 sets, 164 real roots): every root that comes back is within
 * 0.4 x 2^-52 / sigma of an exact root (sigma = smallest singular value of the full system's Jacobian): |E - E_k| <= 1.1e-13
 * on general, forward, sideways, rotating and wide-angle sets (sigma 7e-5 .. 7e-2), <= 5.6e-13 on planar and 1.9e-13 on
 * fronto-parallel ones (sigma 2e-5 .. 2e-3); without the refinement 25 of 164 roots were off by more than 1e6 of those
 * units, up to 0.34 in E.  Completeness holds for the search, not for a single sample: every one of the 164 roots is
 * reached through the 256 samples of a round (they draw the same points in many orders), but one solve can miss a
 * root -- on 2 of the 32 sets (both fronto-parallel) it returned 5 of 6: two roots 2e-3 apart in the hidden variable
 * leave the determinant 1e-2 off, both refinements run into the same root, and the same E is then listed twice.
 * Tie rule of the cheirality vote: ties at a non-zero count keep OpenCV's order of preference (R1 = U W V^T before
 * R2 = U W^T V^T, +t before -t, in the labelling of this library's Jacobi SVD).  When all four counts are 0 the choice
 * is a property of E alone: the rotation with the larger trace (the smaller angle), then the t with E = +[t]x R.
 * distance_thresh = 50 (OpenCV's) counts a point only if its depth is under 50 BASELINES in both views, so with a
 * baseline under 2 % of the scene depth every point lies beyond it, all four candidates score 0, n_good = 0 and only
 * the tie rule picks the pose (t is then no more than a sign convention): a bootstrap frame pair must have a baseline
 * over 2 % of the depth of its points.
 * K [batch][9]; pts1, pts2 [batch][n][2] f32 pixels (NaN rows are never inliers); E [batch][9] (unit Frobenius norm,
 * may be NULL), R [batch][9], t [batch][3] (|t| = 1, x2 ~ R x1 + t); inlier_mask [batch][n] u8 (may be NULL). */
int32_t vo_essential_default_params(vo_ess_params* p);
int32_t vo_essential_ransac(vo_ctx* ctx, const double* K, const float* pts1, const float* pts2, int32_t n,
                            const vo_ess_params* prm, double* E, double* R, double* t, uint8_t* inlier_mask,
                            vo_ess_stats* stats);

/* ---- homography of the 2D-2D bootstrap and the two-view degeneracy check -------------------------
 * cv2.findHomography(p1, p2, cv2.RANSAC, 3.0) of OpenCV 4.4, the step the reference's bootstrap names in a comment and leaves out
 * (Pipeline._get_init_state, src/pipeline/pipeline.py:66 "Estimate homography", in front of the camera_pose call of :68): fitted next
 * to the essential matrix it tells a frame pair without a baseline, or of a planar scene, from one whose five-point pose can be
 * trusted (Extractor.bootstrap_check).  Rounds of 256 four-point samples: hypothesis h draws sample4(seed, h, n), the generator of
 * the other two searches; a sample with three collinear points in either view, or one whose four triples do not keep or reverse
 * their orientation together (OpenCV's checkSubset), has no model and still counts; a lane per sample solves the Hartley-normalised
 * 8 x 8 system in float64; a wave per hypothesis counts |x2 - proj(H x1)|^2 <= threshold^2 in float64 (OpenCV: float32); most
 * inliers win, ties to the smallest h, at least 4; the bound is RANSACUpdateNumIters with 4 model points.  The mask is the winner
 * H0's and is not recomputed; with n > 4 the inliers are re-fitted by the normalised DLT and refined by at most refine_iters
 * Levenberg-Marquardt steps on the forward transfer error (8 parameters in the normalised frame); n = 4 returns H = H0.  Sample
 * draws differ from OpenCV's: statistical parity; the algorithm is defined by tests/homography_model.py.
 * pts1, pts2 [batch][n][2] f32 pixels (NaN rows, and points whose projective w is 0 or not finite, are never inliers); H, H0
 * [batch][9] row-major, unit Frobenius norm, h33 >= 0, x2 ~ H x1 (H0 may be NULL); inlier_mask [batch][n] u8 (may be NULL); stats
 * [batch] (may be NULL).  A sequence without a model: status VO_E_NUMERIC, NaN H and H0, an empty mask; the call returns VO_OK.
 * VO_E_INVALID with nothing enqueued: n < 4, threshold <= 0, confidence outside (0, 1), max_iters < 1, refine_iters outside 0..100. */
int32_t vo_homography_default_params(vo_hom_params* p);
int32_t vo_homography_ransac(vo_ctx* ctx, const float* pts1, const float* pts2, int32_t n, const vo_hom_params* prm,
                             double* H, double* H0, uint8_t* inlier_mask, vo_hom_stats* stats);

/* ---- pose from the homography: what the bootstrap does when the degeneracy check fires ---------------
 * cv2.decomposeHomographyMat(H, K) followed by cv2.filterHomographyDecompByVisibleRefpoints, with the two visibility tests counted
 * per candidate instead of all-or-nothing (an outlier does not veto a candidate), a ranking, and a verdict on whether the pair can
 * decide (ORB-SLAM ReconstructH, COLMAP).  The algorithm is defined by tests/hpose_model.py.
 * G = K^-1 H K (K read as fx, fy, cx, cy), negated if det G < 0: both cameras on the same side of the plane, a property of H alone, so
 * H may come at any scale and sign.  One-sided Jacobi SVD of G in float64 (the condition is never squared; s^2 - 1 enters as
 * (s - 1)(s + 1)), singular values divided by the middle one: s1 >= 1 >= s3.  The solutions of G / s2 = R + (t / d) n^T with R in
 * SO(3), |n| = 1 are two pairs {(R, t, n), (R, -t, -n)}: four entries, also where the pairs coincide (t || n: s1 = 1 or s3 = 1;
 * n_distinct = 2).  s1 - s3 <= 2^-26 (below it the directions of t and n carry fewer than about 26 bits) is a rotation: one solution,
 * R the rotation nearest G / s2, t = n = 0, every vote 0.
 * Votes over the points i < n with finite coordinates, m = ((p - c) / f, 1) in float64 as vo_essential_ransac normalises:
 * n_good[k] counts the points of the mask with n_k . m1 > 0 and (R_k n_k) . m2 > 0; n_off[k] the points outside the mask whose
 * squared Sampson distance under E_k = [t_k / |t_k|]x R_k is <= (threshold / ((fx + fy) / 2))^2 (off-plane points tell the true
 * candidate from the false one; with a NULL mask there are none).  Rank: the viable candidates (n_good >= ratio x max n_good) first;
 * then n_off descending; then, with a hint, n_k . hint descending; then n_good descending; then trace R, n_z, n_y, n_x descending,
 * properties of the solution, so the labelling of the SVD never shows.  ambiguous = 1 iff no hint was given and the best candidate
 * has a viable rival distinct from it (the first in rank order) fewer than min_off behind it in n_off: a plane seen by a moving camera
 * without off-plane points has two solutions that pass every point in both views, and only a prior or a third view tells them apart.
 * vo_homography_decompose: K, H [batch][9] row-major (x2 ~ H x1, pixels); pts1, pts2 [batch][n][2] f32 pixels (NULL with n = 0: the
 * pure cv2.decomposeHomographyMat, every vote 0); mask [batch][n] u8 (NULL: every point is in it); prm NULL: the defaults; R
 * [batch][4][9], t [batch][4][3] (t / d, as cv2 returns it), nrm [batch][4][3] in rank order, entries beyond n_solutions NaN (each
 * may be NULL); stats [batch] (may be NULL).  A sequence without a solution: status VO_E_NUMERIC, NaN outputs; the call returns VO_OK.
 * vo_homography_pose: vo_homography_ransac(pts1, pts2, n, hom_prm) -> H, H0, inlier_mask, hom_stats as that call returns them, with
 * the decomposition of the refined H against the winner's mask enqueued behind the search's last kernel on the same stream: H and
 * the mask are read where they lie on the device, there is one read-back and no host synchronisation in between; the result is that
 * of vo_homography_decompose on the returned H and mask, bit for bit.  A sequence without a homography reports VO_E_NUMERIC in both.
 * VO_E_INVALID with nothing enqueued: ratio outside (0, 1], threshold <= 0 or not finite, min_off < 0, use_hint with a hint that is
 * zero or not finite, n < 0, n > 0 with NULL points, a NULL K or H; for vo_homography_pose also what vo_homography_ransac rejects. */
int32_t vo_homography_pose_default_params(vo_hpose_params* p);
int32_t vo_homography_decompose(vo_ctx* ctx, const double* K, const double* H, const float* pts1, const float* pts2,
                                const uint8_t* mask, int32_t n, const vo_hpose_params* prm, double* R, double* t, double* nrm,
                                vo_hpose_stats* stats);
int32_t vo_homography_pose(vo_ctx* ctx, const double* K, const float* pts1, const float* pts2, int32_t n,
                           const vo_hom_params* hom_prm, const vo_hpose_params* pose_prm, double* H, uint8_t* inlier_mask,
                           double* R, double* t, double* nrm, vo_hom_stats* hom_stats, vo_hpose_stats* pose_stats);

/* ---- fundamental matrix: epipolar verification of matches without intrinsics ----------------------
 * cv2.findFundamentalMat(p1, p2, cv2.FM_RANSAC, 3.0, 0.99) of OpenCV 4.4, next to vo_essential_ransac (which needs K) and
 * vo_homography_ransac.  Rounds of 256 seven-point samples: hypothesis h draws sample7(seed, h, n), the generator of the other
 * searches, with no subset check (OpenCV's FMEstimatorCallback has none: a degenerate sample yields poor models and still counts); a
 * lane per sample Hartley-normalises the seven points, finds the two-dimensional null space of the 7 x 9 system, and keeps every
 * real root of det(a F1 + (1 - a) F2) = 0 (1 or 3) as a model; a system with a larger null space (a repeated point, a sample on a
 * line) has none.  A wave per model counts err <= threshold^2, err = max(d1^2 s1, d2^2 s2) the larger squared point-to-epiline
 * distance; most inliers win, ties to the smallest h, between the models of one sample to the smaller sum of err over the consensus
 * set, at least 7; the bound is RANSACUpdateNumIters with 7 model points.  The mask is the winner F0's and is not recomputed.
 * refit = 0: F = F0; refit = 1 with at least 8 inliers: the normalised eight-point algorithm on the consensus set, rank 2 enforced.
 * Stated deviations from cv2: err in float64 (cv2: float32); for 7 < n < 15 cv2 silently switches to LMedS, this runs RANSAC for
 * every n >= 8; for n = 7 cv2 returns every root stacked as 9 x 3, this returns the winner by the tie rule; cv2 scales F to f33 = 1,
 * this returns unit Frobenius norm (the Python layer divides by f33).  Sample draws differ from OpenCV's: statistical parity; the
 * algorithm is defined by tests/fundamental_model.py.
 * pts1, pts2 [batch][n][2] f32 pixels (NaN rows, and points whose epipolar line has a^2 + b^2 = 0 or a value that is not finite in
 * either view, are never inliers); F, F0 [batch][9] row-major, unit Frobenius norm, the entry of the largest magnitude positive,
 * x2^T F x1 = 0 (F0 may be NULL); inlier_mask [batch][n] u8 (may be NULL); stats [batch] (may be NULL).  A sequence without a model:
 * status VO_E_NUMERIC, NaN F and F0, an empty mask; the call returns VO_OK.
 * VO_E_INVALID with nothing enqueued: n < 7, threshold <= 0 or not finite, confidence outside (0, 1), max_iters < 1, refit outside
 * 0..1. */
int32_t vo_fundamental_default_params(vo_fund_params* p);
int32_t vo_fundamental_ransac(vo_ctx* ctx, const float* pts1, const float* pts2, int32_t n, const vo_fund_params* prm,
                              double* F, double* F0, uint8_t* inlier_mask, vo_fund_stats* stats);

/* ---- Sim(3) / rigid alignment of two 3-D point sets ------------------------------------------------
 * dst ~ s R src + t between two sets of corresponding 3-D points with outliers: two maps of the same landmarks after a re-bootstrap, an
 * estimated trajectory against its ground truth, a loop closure.  Umeyama 1991 / Horn 1987 inside the RANSAC of
 * cv2.estimateAffine3D(src, dst, ransacThreshold = 3.0, confidence = 0.99) and of ORB-SLAM's ComputeSim3, next to the 2D-2D searches
 * above.  Rounds of 256 three-point samples: hypothesis h draws sample3(seed, h, n), the generator of the other searches; a lane per
 * sample forms the centroids and Sigma = 1/3 sum (y_i - yc)(x_i - xc)^T, takes its singular values and vectors by one-sided Jacobi
 * rotations, R = U diag(1, 1, det U det V) V^T (a three-point Sigma has rank 2, so the determinant rule decides every sample and R is a
 * proper rotation also where dst mirrors src), s = tr(D S) / var_x (with_scale = 0: s = 1, Kabsch) and t = yc - s R xc.  A sample with
 * a coordinate that is not finite, with collinear or coincident points in either set
 * (|(b - a) x (c - a)|^2 <= 1e-10 |b - a|^2 |c - a|^2) or, with scale, with s <= 0 or not finite has no model and still counts
 * (stats.degenerate).  A wave per sample counts |y - (s R x + t)|^2 <= threshold^2 in dst's units; most inliers win, ties to the
 * smallest h, at least 3; the bound is RANSACUpdateNumIters with 3 model points.  The mask is the winner's and is not recomputed.
 * refit = 1: Umeyama over the consensus set in two passes (centroids, then central moments about them, a fixed reduction order), unless
 * the set is degenerate -- the second eigenvalue of either set's scatter matrix <= 1e-10 of the first -- or the re-fit is not finite;
 * then, and with refit = 0, the winning sample's model is returned; stats.refit says which.  cost is the sum of squared errors of the
 * consensus set under the returned model.  The algorithm is defined by tests/sim3_model.py.
 * Stated deviations from cv2.estimateAffine3D: the sample draws are this library's, so parity is statistical; the model is a similarity
 * (or a rigid motion), not a 12-parameter affine map; the error is evaluated in float64.
 * Measured on the model against a 40-digit truth (tests/test_sim3_model.py), with kappa = s1 / (s2 + d3) of Sigma's signed singular
 * values: a three-point model lies within SOLVE_FACTOR x 2^-52 x kappa and a re-fit within REFIT_FACTOR x 2^-52 x kappa of the truth
 * (SOLVE_FACTOR = 13, REFIT_FACTOR = 32: 4 x the measured 3.00 and 7.93); the kernels are held to the same bounds against the model
 * (measured on the MI355X: at most 1.84 and 5.7), and results are bitwise reproducible across calls and batch positions.
 * vo_sim3_ransac: src, dst [batch][n][3] f32 (a row with a coordinate that is not finite in either set is never an inlier); prm NULL:
 * the defaults; scale [batch], R [batch][9] row-major, t [batch][3]; model0 [batch][13] = (s, R, t) of the winning sample as found;
 * inlier_mask [batch][n] u8 (of model0); stats [batch]; every output may be NULL.  A sequence without a model: status VO_E_NUMERIC,
 * NaN outputs, an empty mask; the call returns VO_OK.
 * vo_sim3_fit: the finish pass alone, without a search: Umeyama over the rows of mask [batch][n] u8 (NULL: every row) whose
 * coordinates are finite -- the plain least-squares alignment.  vo_sim3_ransac returns, bit for bit, what vo_sim3_fit returns on the
 * mask it reports (stats.refit = 1).  Fewer than 3 rows or a degenerate set: status VO_E_NUMERIC, NaN outputs.
 * VO_E_INVALID with nothing enqueued: n < 3, threshold <= 0 or not finite, confidence outside (0, 1), max_iters < 1, with_scale or
 * refit outside 0..1, a NULL src or dst. */
int32_t vo_sim3_default_params(vo_sim3_params* p);
int32_t vo_sim3_ransac(vo_ctx* ctx, const float* src, const float* dst, int32_t n, const vo_sim3_params* prm, double* scale,
                       double* R, double* t, double* model0, uint8_t* inlier_mask, vo_sim3_stats* stats);
int32_t vo_sim3_fit(vo_ctx* ctx, const float* src, const float* dst, const uint8_t* mask, int32_t n, int32_t with_scale,
                    double* scale, double* R, double* t, vo_sim3_stats* stats);

/* ---- sparse direct image alignment: the frame's pose BEFORE any feature is tracked ---------------
 * The reference has a pose for a new frame only after KLT and cv2.solvePnPRansac (extractor.py:182-186), so its tracker starts every
 * point where it was.  vo_sparse_align gives the 6-DoF pose of the CURRENT frame of the store against the PREVIOUS one directly from the
 * two pyramids and n 3-D points given in the previous camera's coordinates -- the first stage of semi-direct VO (Forster et al., SVO,
 * ICRA 2014, IV-A): 4 x 4 patches around the projected points, photometric error, inverse-compositional Gauss-Newton with Huber
 * weights, coarse to fine.  Projecting the points with it yields start positions for vo_klt_track_init, also for tracks born one frame
 * earlier, and a pose when tracking collapses.  The algorithm is defined by tests/align_model.py, in short:
 *   level l (max_level down to min_level)   f_l = f / 2^l, c_l = c / 2^l (the tracker's p_l = p / (1 << l)); bilinear samples
 *             top = I00 + a (I01 - I00), bot likewise, I = top + b (bot - top) in float32; interior: 4 <= x < w_l - 5, 4 <= y < h_l - 5
 *   reference u = pi_l(X); usable: X finite, X.z > 0, u in the interior; patch offsets {-2, -1, 0, 1}^2; gradient by central
 *             differences of the same bilinear samples; J_p = dpi_l/dX [I | -[X]x] of the patch centre; xi = (translation, rotation)
 *   iteration Y = R X + t, v = pi_l(Y); used: usable, Y.z > 0, v in the interior; r = I_cur(v + o) - I_prev(u + o); weight 1 where
 *             |r| <= huber, else huber / |r| (huber = 0: off); H = sum w J J^T, b = sum w J r, chi = sum w r^2 / (16 n_used) with
 *             J = gx J_p[0] + gy J_p[1]; fewer than min_points used in a level's first iteration: the level is skipped (iters -1);
 *             later, or chi > chi_prev: the previous pose is restored and the level ends; H xi = b by Cholesky (a pivot that is not
 *             positive ends the level, pose kept); T <- T E(xi)^-1 with E = (Rodrigues(omega), v); max(|omega_i|, |v_i| / zbar) < eps
 *             ends the level (zbar: mean depth of the points used in the level's first iteration -- free of the monocular scale)
 *   order     the tests of a linearisation, which is what stats.flags names: too few points (VO_ALIGN_END_POINTS) before chi > chi_prev
 *             (CHI; chi == chi_prev continues), then the pivot (PIVOT), then the step below eps (EPS); the level's last linearisation
 *             ends it by MAX_ITERS.  A point that is not used samples at (8, 8), on a level below 12 pixels in the store's border: its
 *             values reach no sum (tests/test_gpu_align_edges.py runs every exit, levels down to 9 x 6 and the interior's edges)
 * The per-pixel arithmetic is float32, the 16-pixel sums of a point are float32 in a fixed order, everything from there on float64 in
 * a fixed order: a result does not depend on the batch position or on the call.  Against the model the kernel is held to 4 x what
 * the model's own float32 switch moves the pose (tests/test_gpu_align.py).  The basin is about the patch half-width times 2^max_level
 * pixels of image motion: with two levels a 10-pixel motion is outside it.
 * One workgroup per sequence runs a level in one launch on the front-end stream; the call is synchronous like vo_klt_track.
 * K [batch][9] row-major (fx, fy, cx, cy are read); pts3d [batch][n][3] f32 (a NaN row or a row with z <= 0 is never used);
 * rvec0 / tvec0 [batch][3] the initial pose, both NULL = identity; rvec / tvec [batch][3] with x_cur = R(rvec) x_prev + tvec, as
 * vo_pnp_ransac; used_mask [batch][n] u8: the points used in the last kept linearisation of the finest level that ran; stats [batch];
 * rvec, tvec, used_mask and stats may be NULL.  No level ran: stats.status = VO_E_NUMERIC, the pose is the initial one, an empty mask;
 * the call returns VO_OK.
 * Errors, nothing enqueued: fewer than two frames pushed or a step in flight: VO_E_STATE; n > max_pts: VO_E_CAPACITY; VO_E_INVALID for
 * n < 0, a NULL K or pts3d, a level outside the store (max_level = -1: its top level), min_level > max_level, max_iters < 1,
 * min_points < 1, a NaN or negative huber or eps, form outside 0..2, and exactly one of rvec0 / tvec0 NULL.
 * The two structures have no hidden padding: 32 and 56 bytes. */
typedef struct {
  int32_t max_level;         /* -1: the store's top level */
  int32_t min_level;         /* 0 */
  int32_t max_iters;         /* 10, per level */
  int32_t min_points;        /* 10 */
  float   huber;             /* 10 grey levels; 0: no weighting */
  float   eps;               /* 1e-5 */
  int32_t form;              /* 0: the rule; 1: reference patches and gradients kept in a workspace; 2: recomputed every iteration.  Same bits */
  int32_t reserved;          /* 0 */
} vo_align_params;

enum { VO_ALIGN_END_EPS = 1, VO_ALIGN_END_MAX_ITERS = 2, VO_ALIGN_END_CHI = 3, VO_ALIGN_END_PIVOT = 4, VO_ALIGN_END_POINTS = 5 };
typedef struct {
  int32_t status;            /* 0, or VO_E_NUMERIC when no level ran */
  int32_t n_used;            /* points used in the last kept linearisation of the finest level that ran */
  int32_t levels_run;
  int32_t flags;             /* how the finest level that ran ended: VO_ALIGN_END_* */
  int32_t iters[8];          /* linearisations per level; -1: skipped; 0: not asked for */
  float   chi2;              /* chi of that linearisation: mean weighted squared residual, grey levels squared */
  float   zbar;              /* mean depth of the points used in that level's first iteration */
} vo_align_stats;
int32_t vo_align_default_params(vo_align_params* p);
int32_t vo_sparse_align(vo_ctx* ctx, const double* K, const float* pts3d, int32_t n, const double* rvec0, const double* tvec0,
                        const vo_align_params* prm, double* rvec, double* tvec, uint8_t* used_mask, vo_align_stats* stats);

/* ---- recursive depth filter for track candidates ------------------------------------------------
 * The reference turns a candidate corner into a landmark by waiting min_track_length frames and triangulating two views by DLT
 * (extractor.py triangulate_tracks): a candidate carries no depth and no uncertainty while it waits, and the frames between the first and
 * the last view are thrown away.  The complement of vo_sparse_align in semi-direct VO is the depth filter (Forster et al., SVO, ICRA 2014,
 * V; dense: Pizzoli et al., REMODE, ICRA 2014): every candidate (a SEED) holds a Gaussian over the inverse distance mu along its bearing
 * and a Beta(a, b) over its inlier ratio (Vogiatzis and Hernandez 2011), and every later frame with a known pose contributes one
 * measurement.  The algorithm is defined by tests/depth_model.py, in short:
 *   seed      pixel (u, v) of the reference frame, bearing f = normalize(K^-1 (u, v, 1)), a 10 x 10 u8 patch centred on
 *             floor((u, v) + 0.5) (inner 8 x 8: offsets -4..3); mu = 1 / depth_mean, z_range = 1 / depth_min, sigma2 = z_range^2 / 36,
 *             a = b = 10; a patch that leaves the image, or a pixel that is not finite: ok = 0 and the seed is flagged diverged
 *   update    against the store's CURRENT frame under x_cur = R x_ref + t of the seed's ref_id.  The exits in order: inactive (a state
 *             value not finite, sigma2 <= 0, mu <= 0, a flag set, (u, v) outside the image, ref_id outside the pose list, a pose entry
 *             not finite or beyond 1e15); the segment A, B, C = pi(X(1 / (mu + s))), pi(X(1 / max(mu - s, 1e-8))), pi(X(1 / mu)) with
 *             s = sqrt(sigma2), X(d) = (R f) d + t: one of them not in front: invisible; n_steps = ceil(max |B - A|) > max_steps: long;
 *             candidates k = 0..n_steps at floor(A + k (B - A) / n_steps + 0.5), scored where the 10 x 10 patch is inside the image by
 *             S = 64 sum (p - q)^2 - (sum p - sum q)^2 (64 x ZMSSD, exact); smallest S, ties to the smallest k; none scored:
 *             invisible; S > 64 max_score: outlier; n_steps < 2: no search, from floor(C + 0.5).  Then 1-D inverse-compositional
 *             Gauss-Newton on (offset along the segment, mean difference) with the aligner's bilinear form (det H not positive, leaving
 *             the image or no convergence: outlier); triangulation of [R f, -f_cur] (d_ref, d_cur) = -t by its normal equations
 *             (determinant below 1e-6 |t|^2 or d_ref <= 0: degenerate); the measurement noise tau from px_noise pixels by the law of
 *             sines; the moment-matched Gaussian x Beta update.  An outlier is b += 1.  Converged: sqrt(sigma2) < z_range / conv_ratio;
 *             diverged: a / (a + b) < min_inlier; a flagged seed is inactive from the next call on
 * The reference patch is not warped: the filter is for the short baselines of consecutive frames, as in REMODE.  Level 0 only.
 * The per-pixel alignment arithmetic and its 64-pixel sums are float32 in a fixed order, everything else float64: a result does not
 * depend on the batch position or on the call.  Against the model the kernel is held to 4 x what the model's own float32 switch moves
 * each output (tests/test_gpu_depth.py).  One wave per seed, every sequence in one launch on the front-end stream; both calls are
 * synchronous like vo_klt_track.
 * vo_depth_seed_init: uv [batch][n][2] f32, depth_mean / depth_min [batch]; reads the store's current frame; seeds [batch][n],
 * patches [batch][n][100] u8, ok_mask [batch][n] u8 (may be NULL) come back.
 * vo_depth_update: K [batch][9] row-major; poses [batch][n_ref][6] (rvec, tvec as vo_pnp_ransac); seeds [batch][n] in and out;
 * result [batch][n] u8 (VO_DEPTH_*), match_uv [batch][n][2] f32 (where the seed is in the current frame: the best candidate of an
 * outlier without a match, else the last alignment step; NaN where none was reached), z [batch][n] f64 (the triangulated distance, else
 * NaN), stats [batch]; prm NULL = the defaults; result, match_uv, z and stats may be NULL.
 * Errors, nothing enqueued: no frame pushed or a step in flight: VO_E_STATE; n > max_pts: VO_E_CAPACITY; VO_E_INVALID for n < 0, a NULL
 * required pointer, n_ref < 1, max_steps outside 1..128, max_iters < 1, max_score outside 0..4161600, an eps_align, px_noise,
 * conv_ratio or min_inlier that is not finite or is negative, conv_ratio = 0 (every seed would be converged), a depth_mean or depth_min
 * that is not finite and positive.  A ref_id outside 0..n_ref - 1 is the seed's VO_DEPTH_SKIP_INACTIVE, not an error.
 * The three structures have no hidden padding: 32, 56 and 40 bytes. */
typedef struct {
  int32_t max_steps;         /* 128: the longest segment searched, in pixels (1..128) */
  int32_t max_iters;         /* 10: alignment iterations */
  int32_t max_score;         /* 300 * 64: the largest ZMSSD sum of a match, here an rms of 17 grey levels (0..4161600).  SVO's 2000 per pixel
                                is for warped patches over wide baselines; without a warp it admits half-covered patches (EXPERIMENTS.md) */
  float   eps_align;         /* 0.03 pixels */
  float   px_noise;          /* 1 pixel */
  float   conv_ratio;        /* 200 */
  float   min_inlier;        /* 0.1 */
  int32_t reserved;          /* 0 */
} vo_depth_params;

enum { VO_DEPTH_UPDATED = 0, VO_DEPTH_OUTLIER_NOMATCH = 1, VO_DEPTH_OUTLIER_ALIGN = 2, VO_DEPTH_SKIP_INVISIBLE = 3, VO_DEPTH_SKIP_LONG = 4,
       VO_DEPTH_SKIP_DEGENERATE = 5, VO_DEPTH_SKIP_INACTIVE = 6 };
/* vo_depth_seed.flags: the two flags, and from bit VO_DEPTH_OBS_SHIFT on the number of measurements (updates and outliers) taken */
enum { VO_DEPTH_CONVERGED = 1, VO_DEPTH_DIVERGED = 2, VO_DEPTH_OBS_SHIFT = 8 };
typedef struct {
  double  mu, sigma2, a, b, z_range;
  float   u, v;
  int32_t ref_id;
  int32_t flags;
} vo_depth_seed;
typedef struct {
  int32_t counts[7];         /* seeds per result code of this call */
  int32_t converged;         /* seeds flagged converged after it */
  int32_t diverged;
  int32_t reserved;
} vo_depth_stats;
int32_t vo_depth_default_params(vo_depth_params* p);
int32_t vo_depth_seed_init(vo_ctx* ctx, const float* uv, int32_t n, const double* depth_mean, const double* depth_min, int32_t ref_id,
                           vo_depth_seed* seeds, uint8_t* patches, uint8_t* ok_mask);
int32_t vo_depth_update(vo_ctx* ctx, const double* K, const double* poses, int32_t n_ref, vo_depth_seed* seeds, const uint8_t* patches,
                        int32_t n, const vo_depth_params* prm, uint8_t* result, float* match_uv, double* z, vo_depth_stats* stats);

/* ---- SIFT features (SURVEY.md 8f "next" row 4, feature part) -----------------------------------
 * Replaces cv2.SIFT_create(nfeatures=1000).detect(img, mask) + .compute(img, kps) in
 * Extractor.extract(detector='custom', describe=True) (src/extractor/extractor.py:26-28, 114-122; the two bootstrap
 * frames of Pipeline._get_init_state, src/pipeline/pipeline.py:48-49): doubled base image, Gaussian / DoG scale space
 * (3 layers per octave, sigma 1.6), 26-neighbour extrema, quadratic refinement with contrast (0.04) and edge (10)
 * tests, orientation histogram peaks, removeDuplicatedSorted + retainBest(nfeatures), 4 x 4 x 8 descriptors scaled to
 * 0..255.  The float32 operation order is defined by oracle/sift_oracle.py; the algorithm is pinned to an independent
 * float64 model and to scale-space truths (tests/sift_model.py, tests/test_gpu_sift_model.py).  Conventions, as in
 * OpenCV 4.4: a feature at pixel centre (cx, cy) is reported at (cx + 0.25, cy + 0.25) -- createInitialImage doubles
 * the image with INTER_LINEAR, whose sample d sits at (d + 0.5) / 2 - 0.5 of the source, and the halved keypoints keep
 * that quarter pixel (later OpenCV: enable_precise_upscale); angle = direction of the intensity gradient in degrees,
 * from +x towards +y with y pointing down, atan2(gy_down, gx) mod 360.  Unpinned without OpenCV itself: the float
 * summation order inside its SIMD filters, and compute() rebuilding the pyramid from the keypoints' lowest octave
 * when no first-octave keypoint survives (here the descriptors always come from the detection pyramid).
 * img [batch][height][stride] u8 (the context's image size); mask the same layout or NULL (0 = drop the keypoint);
 * kps [batch][max_out]; desc [batch][max_out][128] f32; n_out [batch].  VO_E_CAPACITY if max_out is too small. */
int32_t vo_sift_detect_compute(vo_ctx* ctx, const uint8_t* img, int32_t stride, const uint8_t* mask, int32_t nfeatures,
                               int32_t max_out, vo_sift_kp* kps, float* desc, int32_t* n_out);

/* ---- multi-scale ORB features -------------------------------------------------------------------
 * The reference's Extractor names two feature methods, 'sift' and 'orb' (src/extractor/extractor.py:26-33: cv2.ORB_create(); :114-122 detect +
 * compute; :144-145 the 1-NN Hamming match).  This is the 'orb' one: FAST-9/16 corners on a scale pyramid, Harris re-ranking, per-level quotas,
 * orientation by intensity centroid and the steered 256-bit BRIEF of the section above.  Neither OpenCV nor its learned table is part of this
 * project: parity with cv2.ORB is not pinned, the numpy model tests/orb_model.py is the definition, and the kernels equal it bit for bit
 * (integer arithmetic or single IEEE operations in a fixed order).
 *   geometry   float64 on the host: s_l = scale_factor^l (pow), w_l = rint(w / s_l), h_l = rint(h / s_l), half to even; the reported scale is
 *              (float)s_l.  A level with w_l < 1 or h_l < 1 has no pixels.
 *   quotas     OpenCV's rule in float64: f = 1 / scale_factor, nd = nfeatures (1 - f) / (1 - f^nlevels); levels 0 .. nlevels-2 get rint(nd) and
 *              nd *= f after each; the last level gets max(nfeatures - sum, 0).  nlevels = 1: the single level gets nfeatures.
 *   pyramid    level 0 is the image, level l is resized from level l-1 by fixed-point bilinear interpolation: per axis destination d samples
 *              the source at fx = (d + 0.5) (src / dst) - 0.5 in float64, i0 = floor(fx), a = rint((fx - i0) 2048), both taps i0 and i0 + 1
 *              clamped to [0, src-1]; pixel = (sum of the four products of the (2048 - a, a) weights + 2^21) >> 22.  The (tap, weight) tables
 *              are made on the host (like the undistortion map and the CLAHE table), so no float enters the kernel.
 *   candidates strict 3 x 3 maxima of the FAST score (section "Shi-Tomasi re-detection": fast_threshold) of the level with 31 <= lx < w_l - 31
 *              and 31 <= ly < h_l - 31 (edge_threshold = 31, fixed); under a mask those with
 *              mask[min(h-1, rint((float)ly * (float)s_l))][min(w-1, rint((float)lx * (float)s_l))] != 0.
 *   retention  OpenCV's retainBest, ties kept, both rules sets: keep i iff fewer than 2 quota_l candidates of the level have a strictly greater
 *              FAST score; then, among those, iff fewer than quota_l have a strictly greater Harris response.  A level can return more than
 *              its quota.
 *   Harris     ORB's HarrisResponses over the 7 x 7 block centred on the keypoint: Ix = 2 (I(x+1,y) - I(x-1,y)) + (I(x+1,y-1) - I(x-1,y-1)) +
 *              (I(x+1,y+1) - I(x-1,y+1)), Iy its transpose; a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy in int32; in float32, every operation
 *              rounded on its own, ((fa fb - fc fc) - (0.04f (fa + fb)) (fa + fb)) * sc4, sc4 = (float)((1 / (4 * 7 * 255))^4); harris_k = 0.04f, fixed.
 *   describe   angle and descriptor of the section above on the level image at (lx, ly); the 31-pixel edge implies its 24-pixel margin.
 *   output     per sequence by level ascending, response descending, ly ascending, lx ascending; x = (float)lx * (float)s_l, y likewise,
 *              size = 31.0f * (float)s_l, octave = l.
 * Not cv2.ORB: the sampling table (the caller's, or the generated default), no fastAtan2 (the angle is atan2 in float64 and never enters the
 * descriptor), the integer 7-tap Gaussian in place of GaussianBlur(7 x 7, 2), plain fixed-point bilinear resizing in place of INTER_LINEAR_EXACT,
 * and the mask sampled at the keypoint's level-0 position instead of being resized per level.
 * Kernels (csrc/vo_orb.hip): one resize launch per level above 0; then a fixed number of launches, each covering every level and sequence
 * through a tile-to-level table: FAST score, strict maxima into candidate lists and a 256-bin score histogram per (sequence, level), the FAST
 * cut read off the histogram, Harris of the survivors, retention and output position by counting over all pairs of a (sequence, level), one
 * wave per keypoint to describe.  Capacities: 65536 candidates and 8192 rows behind the FAST cut per (sequence, level); beyond either, and
 * when a sequence has more than max_out keypoints, the call returns VO_E_CAPACITY and writes none of its outputs.  Nothing is truncated.
 *   vo_orb_params          nfeatures >= 1 (500); scale_factor in (1, 2] (1.2); nlevels 1..8 (8); fast_threshold 1..254 (20); edge_threshold
 *                          must be 31 and harris_k 0.04f.  vo_orb_default_params fills it.  Anything else: VO_E_INVALID, nothing enqueued.
 *   vo_orb_detect_compute  synchronous.  img [batch][height][stride] u8 (the context's image size), mask the same layout or NULL; prm NULL = the
 *                          defaults; pattern NULL = the default table, else checked as vo_set_brief checks it; kps [batch][max_out],
 *                          desc [batch][max_out][32] u8, n_out [batch].  The pyramid (about 3.3 w h bytes per sequence at 1.2, every level inside
 *                          a 32-pixel border so that no tile load leaves the allocation) is reserved by the first call.
 *   vo_orb_levels_read     of the last call: w_l, h_l, scale_l, quota_l [8] each (zeros beyond nlevels), n_l [batch][8] the keypoints each level
 *                          returned (any may be NULL).  VO_E_STATE before the first successful call.
 *   vo_orb_level_image_read  level `level` of sequence `seq` of the last call's pyramid, out [h_l][w_l] u8. */
typedef struct {
  int32_t nfeatures;         /* 500 */
  int32_t nlevels;           /* 8 */
  double  scale_factor;      /* 1.2 */
  int32_t fast_threshold;    /* 20 */
  int32_t edge_threshold;    /* 31, fixed */
  float   harris_k;          /* 0.04f, fixed */
  int32_t _pad;
} vo_orb_params;             /* 32 bytes */
typedef struct {
  float   x, y;              /* pt, pixels of the input image */
  float   size;              /* 31 * scale of the level */
  float   angle;             /* degrees, [0, 360) */
  float   response;          /* Harris response on the level */
  int32_t octave;            /* pyramid level */
  int32_t lx, ly;            /* integer pixel on the level */
} vo_orb_kp;                 /* 32 bytes */
int32_t vo_orb_default_params(vo_orb_params* p);
int32_t vo_orb_detect_compute(vo_ctx* ctx, const uint8_t* img, int32_t stride, const uint8_t* mask, const vo_orb_params* prm,
                              const int8_t* pattern, int32_t max_out, vo_orb_kp* kps, uint8_t* desc, int32_t* n_out);
int32_t vo_orb_levels_read(vo_ctx* ctx, int32_t* w_l, int32_t* h_l, float* scale_l, int32_t* quota_l, int32_t* n_l);
int32_t vo_orb_level_image_read(vo_ctx* ctx, int32_t seq, int32_t level, uint8_t* out);

/* ---- descriptor matching (SURVEY.md 8f "next" row 4, matching part) -----------------------------
 * Replaces cv2.BFMatcher().knnMatch(desc_1, desc_2, k=2) in Extractor.match (src/extractor/extractor.py:134-145;
 * match_lists :147-154, Pipeline._get_init_state src/pipeline/pipeline.py:52): for every query descriptor the two
 * nearest train descriptors under the L2 norm, ordered by (distance, train index).  The ratio test stays with the caller.
 * desc1 [batch][n1][dim], desc2 [batch][n2][dim] f32; idx [batch][n1][2] (-1 = no such neighbour), dist [batch][n1][2] f32. */
int32_t vo_match_knn2(vo_ctx* ctx, const float* desc1, int32_t n1, const float* desc2, int32_t n2, int32_t dim,
                      int32_t* idx, float* dist);
/* The reference's 'orb' branch, self._matcher.match(desc_1, desc_2) (src/extractor/extractor.py:144-145), over binary descriptors:
 * cv2.BFMatcher(NORM_HAMMING).knnMatch(k = 2) -- for every query the two train rows of least bit distance, ordered by (distance, train
 * index); column 0 is the 1-NN match.  desc1 [batch][n1][nbytes], desc2 [batch][n2][nbytes] u8; nbytes a multiple of 4 in 4..64, else
 * VO_E_INVALID; idx [batch][n1][2] (-1 = no such neighbour), dist [batch][n1][2] i32 (INT32_MAX for an empty slot). */
int32_t vo_match_hamming_knn2(vo_ctx* ctx, const uint8_t* desc1, int32_t n1, const uint8_t* desc2, int32_t n2, int32_t nbytes,
                              int32_t* idx, int32_t* dist);

/* ---- guided descriptor matching: window and epipolar gates, ratio test, cross-check ---------------
 * The second matching pass of a detect / match / verify front end: the two matchers above, with every pair outside a search window or an
 * epipolar band excluded before a descriptor byte is touched, and the decisions on which neighbour to keep (Lowe's ratio test, a distance
 * ceiling, cv2.BFMatcher(crossCheck=True)'s mutual-nearest rule) made on the device.  OpenCV has no guided matcher: the numpy model
 * tests/gmatch_model.py is the definition, and the kernels (csrc/vo_match.hip) equal it bit for bit.
 *   admitted(i, j), for i < counts1[b] and j < counts2[b]:
 *     window (gate bit 0)    c = centers[i], or pts1[i] where centers is NULL; dx = (double)pts2[j].x - (double)c.x, dy likewise;
 *                            (dx dx + dy dy) <= radius radius.  Any NaN makes it false.
 *     epipolar (gate bit 1)  both squared point-to-epiline distances of (pts1[i], pts2[j]) under F are at most epi_dist epi_dist, in the
 *                            float64 expressions of the consensus test of vo_fundamental_ransac (one device function, vo_epi_dev.h): a pair
 *                            admitted at epi_dist = t is a pair that search counts as an inlier of F at threshold t.  A value that is not
 *                            finite (a NaN position, a line with a^2 + b^2 = 0) is never admitted.
 *     both bits: both hold.  gate 0: every existing pair is admitted.
 *   distances  those of the matchers above, bit for bit: the popcount; sqrtf((float)acc), acc the float64 sum in ascending k.
 *   per query i   idx[i][0..1], dist[i][0..1]: the two nearest admitted train rows by (distance, train index); an empty slot is -1 with
 *                 INT32_MAX or +inf.  n_admitted[i]: the number of admitted train rows.
 *   per train row j, with cross_check   rbest[j]: the nearest admitted query by (distance, query index), or -1.  Without: -1.
 *   match[i] = idx[i][0] iff  a nearest row exists,  (double)d0 <= max_dist,  ratio == 1 or there is no second admitted neighbour or
 *              (double)d0 < ratio * (double)d1 (one float64 product: Extractor.match's comparison),  and cross_check == 0 or
 *              rbest[idx[i][0]] == i;  else -1.  The ratio test is not applied on the reverse side.
 * desc1 [batch][n1][nbytes | dim], desc2 [batch][n2][nbytes | dim] as above; pts1 [batch][n1][2], pts2 [batch][n2][2], centers
 * [batch][n1][2] f32 pixels; F [batch][9] row-major with x2^T F x1 = 0 (vo_fundamental_ransac's convention); counts1, counts2 [batch]: rows
 * at or beyond a sequence's count do not exist for it (their outputs are the empty ones), NULL = n1 / n2 for every sequence, 0 is valid.
 * prm NULL = the defaults.  idx, dist [batch][n1][2], n_admitted, match [batch][n1], rbest [batch][n2]; all but match may be NULL.
 * Synchronous on the context's stream.  VO_E_INVALID with nothing enqueued and no output written: a NULL descriptor set or match, n1 < 1,
 * n2 < 1, nbytes / dim outside the rules above, gate outside 0..3, cross_check outside 0..1, a gate bit whose distance is <= 0 or not
 * finite, gate != 0 without pts1 and pts2, bit 1 without F, ratio outside (0, 1], max_dist NaN or negative, a count outside 0..n. */
typedef struct {
  int32_t gate;         /* bit 0: window, bit 1: epipolar; 0 = every pair admitted */
  int32_t cross_check;  /* 0 / 1 */
  double  radius;       /* window gate, pixels */
  double  epi_dist;     /* epipolar gate, pixels */
  double  ratio;        /* (0, 1]; 1 = no ratio test */
  double  max_dist;     /* keep only d0 <= max_dist; +inf = off */
} vo_gmatch_params;     /* 40 bytes */
int32_t vo_gmatch_default_params(vo_gmatch_params* p);   /* gate 0, cross_check 0, radius 0, epi_dist 0, ratio 1, max_dist +inf */
int32_t vo_match_guided_hamming(vo_ctx* ctx, const uint8_t* desc1, int32_t n1, const uint8_t* desc2, int32_t n2, int32_t nbytes,
                                const float* pts1, const float* pts2, const float* centers, const double* F,
                                const int32_t* counts1, const int32_t* counts2, const vo_gmatch_params* prm,
                                int32_t* match, int32_t* idx, int32_t* dist, int32_t* n_admitted, int32_t* rbest);
int32_t vo_match_guided_l2(vo_ctx* ctx, const float* desc1, int32_t n1, const float* desc2, int32_t n2, int32_t dim,
                           const float* pts1, const float* pts2, const float* centers, const double* F,
                           const int32_t* counts1, const int32_t* counts2, const vo_gmatch_params* prm,
                           int32_t* match, int32_t* idx, float* dist, int32_t* n_admitted, int32_t* rbest);

/* ---- device-resident track table (SURVEY.md 8f "next" row 3) -----------------------------------
 * The bookkeeping Extractor.extend_tracks / extend_landmarks / extract do on Python lists of Keypoint objects
 * (src/extractor/extractor.py:38-88, 90-132; src/state/keypoint.py:4-21), as a structure of arrays in HBM: per
 * sequence an ORDERED list (survivors keep their order, detections are appended) of uv (the resident point set),
 * uv_first, t_first, t_total, a stable tag, and a ring of the last 32 positions by absolute frame index.
 *   vo_tracks_seed    initial tracks born at frame t (t_total = 1, history = [uv]);  pts [batch][n][2]
 *   vo_tracks_track   KLT prev -> cur of every live track, then the reference's rule: keep iff 0 <= x <= W and
 *                     0 <= y <= H (ends included; KLT status ignored, bidirectional test off: pipeline.py:98-100) -- and, with a
 *                     finite vo_set_fb_check threshold, the forward-backward check passed (the true bidirectional test);
 *                     survivors: uv, t_total + 1, history append; the others go to the dead list        (async)
 *   vo_tracks_detect  exclusion discs at the live tracks + Shi-Tomasi on the current frame, up to max_new corners per
 *                     sequence appended as tracks born at t (extractor.py:103-132)                      (async)
 *   vo_tracks_read    synchronous read-back: n / n_dead [batch]; uv, uv_first [batch][max_pts][2]; t_first, t_total,
 *                     tag, dead_tag [batch][max_pts]; any pointer may be NULL
 *   vo_tracks_obs     the bundle adjuster's observation table of the live tracks (bundle_adjuster.py:150-158 with
 *                     t_latest = t_now): obs [batch][window][max_pts][2] f64, slot s <-> frame t_now - s, NaN = not
 *                     observed -- the layout vo_ba_upload / vo_ba_adjust take (N = max_pts)
 * Counts differ per sequence of a batch; they stay on the device and the KLT / disc kernels skip the rest. */
int32_t vo_tracks_seed(vo_ctx* ctx, const float* pts, int32_t n, int32_t t);
int32_t vo_tracks_track(vo_ctx* ctx, int32_t t, const vo_klt_params* prm);
int32_t vo_tracks_detect(vo_ctx* ctx, int32_t t, int32_t mask_radius, const vo_st_params* st, int32_t max_new);
int32_t vo_tracks_read(vo_ctx* ctx, int32_t* n, float* uv, float* uv_first, int32_t* t_first, int32_t* t_total,
                       int32_t* tag, int32_t* n_dead, int32_t* dead_tag);
int32_t vo_tracks_obs(vo_ctx* ctx, int32_t t_now, int32_t window, double* obs);
/* the same table written into the RESIDENT BA problem (uploaded with N = max_pts landmarks): no host round trip (async) */
int32_t vo_ba_obs_from_tracks(vo_ctx* ctx, int32_t t_now);

/* ---- closed-loop Pipeline.step on the device (SURVEY.md 8f "next" row 3, the State half) ---------------------------
 * The whole per-frame state the reference keeps in Python lists of objects -- State(landmarks, landmarks_kp, candidates_kp,
 * trajectory) (src/state/state.py:4-10) and Pipeline._landmarks_dead / _landmarks_kp_dead (src/pipeline/pipeline.py:31) -- as
 * device tables, and Pipeline.step (pipeline.py:92-167) as ONE enqueue per frame with every data dependence on the device:
 *   TRACK        pyramid + KLT of all landmark and candidate keypoints, the keep rule and bookkeeping of
 *                Extractor.extend_tracks / extend_landmarks (extractor.py:38-88), what dies goes to the dead lists (pipeline.py:98-103);
 *                with a finite vo_set_fb_check threshold the tracking runs the forward-backward check and a point that fails it dies too
 *   POSE         RANSAC-P3P pose from the landmarks' 3-D points and tracked pixels (extractor.py:174-191), non-inliers to the dead
 *                lists (pipeline.py:124-137), pose appended to the trajectory (:140)
 *   TRIANGULATE  Extractor.triangulate_tracks (extractor.py:193-277): candidates with t_total >= min_track_length leave the
 *                candidate list, DLT between their first and newest observation, cheirality + reprojection filters
 *                (triangulate.py:87-111), the per-group gate of extractor.py:231-240, promotion to landmarks
 *   ADJUST       BundleAdjuster.adjust (bundle_adjuster.py:127-215): dead landmarks whose track lies inside the window are
 *                appended to the state's lists again AS THE SAME OBJECTS (:142-150), observation table from the keypoint
 *                histories (:153-158), x0 from the landmark positions and the window's poses (:165-176), LM solve, positions and
 *                poses written back (:197-213)
 *   DETECT       exclusion discs at every keypoint of the state + Shi-Tomasi, corners appended as candidates (pipeline.py:159-163)
 * Object identity matters in the reference (adjust appends without copying, extend_landmarks deep-copies the keypoint but keeps the
 * landmark object, Pipeline.step deep-copies what dies): the tables are OBJECT rows with stable indices -- K rows (Keypoint:
 * t_first, t_total, uv_first, uv, history length, ring of the last 32 history entries by index) and L rows (Landmark: t_latest, p) --
 * plus ordered lists of row indices (candidates [K]; landmarks [(L, K, keypoint-shared-with-a-dead-entry)]; dead [(L, K)]), so
 * several list entries can refer to one object exactly as in the reference.  Dead entries that can never be resurrected again
 * are dropped and counted.  oracle/pipe_oracle.py restates the algorithm; tests/test_gpu_pipe.py compares the tables with the
 * reference's loop over Python objects frame by frame.
 * Capacity: candidates + landmarks <= max_pts (they share the KLT point buffer), dead list <= max_pts, object rows 4 x max_pts.
 * When a list is full, detections / promotions / resurrections are cut in list order and the record's `overflow` bits say so
 * (the reference's lists are unbounded).
 * Frames come from the resident sequence (vo_seq_upload) by index, or frame_idx = -1: the caller has pushed the frame
 * (vo_frame_push).  Up to VO_PIPE_INFLIGHT steps may be enqueued before the oldest record is fetched; nothing else crosses
 * the bus per frame. */
typedef struct {
  int32_t ba_window;          /* 4    pipeline.py:19  (<= 20) */
  int32_t min_track_length;   /* 3    pipeline.py:147 */
  int32_t mask_radius;        /* 7    pipeline.py:162 (min_kp_dist) */
  int32_t max_new;            /* 1000 corners appended per frame (maxCorners, extractor.py:21) */
  int32_t pnp_blind_batches;  /* 4    batches of P3P hypotheses (32, then 256 each) enqueued per frame (they exit early once the RANSAC bound is reached) */
  int32_t ba_budget;          /* LM iterations enqueued per frame, <= ba.max_iters (they exit early once the LM has stopped) */
  int32_t resurrect;          /* 1: as the reference -- adjust appends dead landmarks whose track lies inside the window to the state's lists again
                                 (bundle_adjuster.py:142-150).  With the reference's window of 4 that is a handful per frame;
                                 with a window of 10 every young death comes back every frame, and again for every copy that dies again, until the
                                 table holds little else (measured: bench.py --workload pipeline).  0: dead landmarks stay dead. */
  int32_t reserved;
  double  max_reproj_err;     /* 2.0  pipeline.py:23 (PnP consensus and triangulation filter) */
  double  min_bearing_angle;  /* 0.5  pipeline.py:24 */
  vo_klt_params klt;
  vo_st_params  st;
  vo_ba_params  ba;
  vo_pnp_params pnp;
} vo_pipe_params;

/* what comes back per sequence and frame */
typedef struct {
  int32_t t;                  /* step index after this frame (Pipeline._t_step) */
  int32_t status;             /* 0, or VO_PIPE_* bits: the sequence stopped at the frame that set them */
  int32_t overflow;           /* capacity policy acted: 1 dead list, 2 promotion, 4 resurrection, 8 detection, 16 Shi-Tomasi candidate capacity */
  int32_t n_landmarks, n_candidates;      /* len(state._landmarks), len(state._candidates_kp) after the frame */
  int32_t n_dead, n_dead_total;           /* dead entries kept on the device / ever (= len(Pipeline._landmarks_dead)) */
  int32_t n_tracked;                      /* keypoints that went into the KLT of this frame */
  int32_t pnp_inliers, pnp_hypotheses, pnp_bound_reached;
  int32_t n_ripe, n_new, n_resurrected, n_detected;
  int32_t ba_landmarks, ba_observations, ba_iters, ba_accepted, ba_status, ba_done;   /* ba_done 0: the budget cut the solve */
  int32_t t_final;            /* step whose pose has just left the BA window (t - ba_window + 1, or -1): H_final will not change any more */
  double  ba_cost0, ba_cost;
  double  H[12];              /* pose of this frame AFTER the adjust: rows of [R | t], world -> camera (later adjusts refine it while it is in the window) */
  double  H_final[12];        /* pose of step t_final: collecting these gives the trajectory the reference ends up with (state._trajectory) */
} vo_pipe_record;

enum { VO_PIPE_LOST = 1, VO_PIPE_CAPACITY = 2, VO_PIPE_GROUPS = 4 };   /* LOST: the 3D-2D pose found no consensus (the reference crashes there); CAPACITY: object rows exhausted; GROUPS: a ripe candidate was born more than 32 frames ago (its pose has left the trajectory ring) */
enum { VO_PIPE_TRACK = 1, VO_PIPE_POSE = 2, VO_PIPE_TRIANGULATE = 4, VO_PIPE_ADJUST = 8, VO_PIPE_DETECT = 16, VO_PIPE_ALL = 31,
       /* the two halves of TRACK's bookkeeping as the reference calls them (extractor.py:38-59 then :61-88): VO_PIPE_TRACK | VO_PIPE_TRACK_CANDIDATES
          = pyramid + KLT of every keypoint + extend_tracks; then VO_PIPE_TRACK_LANDMARKS alone = extend_landmarks on the same tracked set (the
          step counter advances here).  Neither bit: both halves (the closed loop).  Used by the object boundary, vo_mi355x/lazy.py */
       VO_PIPE_TRACK_CANDIDATES = 32, VO_PIPE_TRACK_LANDMARKS = 64,
       /* a stage-wise caller: rows that left the lists in this call are NOT handed out again yet (the free lists are rebuilt by the first later call
          without this bit, normally the frame's DETECT) -- so their contents can still be read back after the call (vo_pipe_rows_read) */
       VO_PIPE_KEEP_FREE_LISTS = 128 };
#define VO_PIPE_INFLIGHT 4
#define VO_PIPE_HIST 32

/* the device tables, for seeding and read-back (all with a leading [batch] dimension; N = max_pts, R = 4 x max_pts rows):
 * K rows: K_TFIRST, K_TTOTAL, K_HISTLEN i32 [R]; K_UV, K_UVFIRST f32 [R][2]; K_HIST f32 [32][R][2] (entry idx in slot idx % 32)
 * L rows: L_TLATEST i32 [R]; L_P f64 [R][3]
 * lists:  CAND i32 [N]; LM_L, LM_K, LM_KSHARED i32 [N]; DEAD_L, DEAD_K i32 [N]
 * COUNTS i32 [32]: [0] n_cand [1] n_lm [2] n_dead [3] n_dead_dropped [4] status [5] t
 * POSES f64 [32][12]: trajectory ring, pose of step t in slot t % 32 */
enum { VO_PIPE_K_TFIRST = 0, VO_PIPE_K_TTOTAL, VO_PIPE_K_HISTLEN, VO_PIPE_K_UV, VO_PIPE_K_UVFIRST, VO_PIPE_K_HIST, VO_PIPE_L_TLATEST,
       VO_PIPE_L_P, VO_PIPE_CAND, VO_PIPE_LM_L, VO_PIPE_LM_K, VO_PIPE_LM_KSHARED, VO_PIPE_DEAD_L, VO_PIPE_DEAD_K, VO_PIPE_COUNTS,
       VO_PIPE_POSES, VO_PIPE_N_TABLES };

int32_t vo_pipe_default_params(vo_pipe_params* p);
/* K [batch][9].  Allocates the tables (empty state, t = 0) and the BA / PnP / DLT workspaces for max_pts landmark slots. */
int32_t vo_pipe_create(vo_ctx* ctx, const double* K, const vo_pipe_params* prm);
int32_t vo_pipe_table_bytes(vo_ctx* ctx, int32_t which, uint64_t* bytes);
int32_t vo_pipe_table_write(vo_ctx* ctx, int32_t which, const void* src);     /* synchronous; needs no steps in flight */
int32_t vo_pipe_table_read(vo_ctx* ctx, int32_t which, void* dst);            /* synchronous */
/* after the tables were written: free rows and the resident point set are rebuilt from the lists */
int32_t vo_pipe_commit(vo_ctx* ctx);
/* one frame; stages = VO_PIPE_ALL, or a subset for stage-wise parity tests (the step counter advances in TRACK)   (async).
 * frame_idx >= 0: frame of the uploaded sequence (vo_seq_upload); < 0: the caller has pushed the frame (vo_frame_push*).
 * Up to VO_PIPE_INFLIGHT steps may be enqueued before the oldest is fetched.  With a side stream (vo_set_side_stream != 0, the
 * default) the re-detection and spawn of frame t and the pyramid + KLT of frame t + 1 (frame_idx >= 0) run beside the bundle
 * adjustment of frame t; results are bit-identical to the one-stream order.  Many sequences: ONE context with a large batch. */
int32_t vo_pipe_step(vo_ctx* ctx, int32_t frame_idx, int32_t stages);
/* the same step with the frame handed over by the host, as the reference's loop does (Pipeline.step(img): src/pipeline/pipeline.py:98,171-172):
 * frames[b] = the new image of sequence b (rows of `stride` bytes).  Upload on the copy stream (see vo_frame_step_host: one gather launch for
 * page-locked images), pyramid + tracking on the side stream behind it -- the overlap of a resident frame.  `stages` must contain VO_PIPE_TRACK.
 * In flight: up to VO_PIPE_INFLIGHT steps, host and resident ones together, as vo_pipe_step.  Every image a step was given, whatever memory holds
 * it (page-locked, registered or pageable), must stay allocated and untouched until vo_pipe_fetch has returned that step.  A refused call
 * (VO_E_STATE: no frame in the store, steps in flight on the gated layout, VO_PIPE_INFLIGHT steps in flight) enqueues nothing. */
int32_t vo_pipe_step_host(vo_ctx* ctx, const uint8_t* const* frames, int32_t stride, int32_t stages);
int32_t vo_pipe_fetch(vo_ctx* ctx, vo_pipe_record* rec /* [batch] */);        /* waits for the OLDEST step not fetched yet */
int32_t vo_pipe_set_ba_budget(vo_ctx* ctx, int32_t budget);
/* Read-backs for the object boundary (vo_mi355x/lazy.py: the reference's Extractor / BundleAdjuster interface, src/extractor/extractor.py:38-277 and
 * src/bundle_adjuster/bundle_adjuster.py:127-215, as views of these tables).  All synchronous, no step may be in flight.
 * lists_read: tables VO_PIPE_CAND .. VO_PIPE_POSES in ONE copy, as they lie on the device -- each [batch][...], each padded to a multiple of 256 bytes.
 * rows_read: object rows by index, kind 0 = K rows -> {i32 t_first, t_total, hist_len, 0; f32 uv[2], uv_first[2]; f32 hist[32][2]} (288 bytes, ring
 * slot order), kind 1 = L rows -> {i32 t_latest, 0; f64 p[3]} (32 bytes); rows [batch][n], n <= max_pts.
 * inliers_read: the consensus mask of the last POSE stage over the landmark list as it was before the pruning, [batch][n]. */
int32_t vo_pipe_lists_bytes(vo_ctx* ctx, uint64_t* bytes);
int32_t vo_pipe_lists_read(vo_ctx* ctx, void* dst);
int32_t vo_pipe_rows_read(vo_ctx* ctx, int32_t kind, const int32_t* rows, int32_t n, void* out);
int32_t vo_pipe_inliers_read(vo_ctx* ctx, uint8_t* mask, int32_t n);

/* ---- forced forms (parity tests, A/B measurements) ---------------------------------------------
 * Every kernel choice the library makes by a rule (which bundle-adjustment family, how a problem is spread over workgroups, which form of the
 * eigenvalue pass, the stream layout's gate ...) can be forced per context; 0 in a field = the rule.  This replaces the process-wide VO_* environment
 * switches of rounds 1-5: the library reads no tuning from the environment any more.  Results do not depend on any of these fields except in the
 * last bits of a bundle adjustment (its partial sums are folded in another order: ~1e-12).  Set it with nothing in flight; the bundle-adjustment
 * fields marked (upload) shape the workspace and take effect at the next vo_ba_upload / vo_ba_upload_bank / vo_pipe_create. */
typedef struct {
  int32_t ba_kernels;          /* (upload) 0: the rule (windows of 9-10 slots, Huber / linear loss: the factored k_ba_build_f<>); 1: lane-per-observation kernels (k_ba_build<>); 2: wave-private kernels (k_ba_build_w<>, windows <= 10) */
  int32_t ba_lanes;            /* (upload) lanes per landmark: 8 = wave-private kernels at windows of 9-10 slots (rule: 5); 16 = lane-per-observation
                                  kernels at windows <= 8 (rule: 8) */
  int32_t ba_threads;          /* (upload) lane-per-observation kernels: workgroup size 256 / 512 / 1024 */
  int32_t ba_pitch_pad;        /* (upload) lane-per-observation kernels: panel pitch = rows + (ba_pitch_pad - 1) doubles */
  int32_t ba_chunks;           /* lane-per-observation kernels: landmark chunks per workgroup */
  int32_t ba_workgroups;       /* wave-private kernels: workgroups per problem in a full launch */
  int32_t ba_workgroup_cap;    /* wave-private kernels: most workgroups a running problem gets once others have finished (rule: 16) */
  int32_t ba_fold;             /* 1: a reduce kernel folds the partial sets; 2: k_ba_solve folds them itself */
  int32_t klt_waves;           /* occupancy bound the tracker is compiled for: 4 / 5 / 6 waves per SIMD (rule: 6) */
  int32_t klt_pair;            /* builds with -DVO_EXPERIMENTS only: 3 / 4 / 5 = two keypoints per wave (k_klt_track2) */
  int32_t st_two_kernels;      /* 1: Sobel + row sums and column sums + eigenvalue as two kernels at block size 31 too (rule: fused) */
  int32_t st_band_rows;        /* rows per band of the fused eigenvalue kernel */
  int32_t st_separate_nms;     /* 1: eigenvalue map through HBM to a separate non-maximum-suppression kernel */
  int32_t st_keep_eig;         /* 1: resident launches keep the eigenvalue map and the mask (vo_shi_tomasi_read after them) */
  int32_t st_host_limit;       /* 1: closed loop: the corner limit of a sequence is not read on the device */
  int32_t xcd_remap_off;       /* 1: plain (block, sequence) order instead of one sequence per XCD */
  int32_t gate_groups;         /* stream layout 2: LM launch groups of frame t ahead of the tracker launch of frame t + 1; -1: none */
  int32_t reserve_cus;         /* stream layout 2: compute units the front-end stream leaves free; -1: none */
  int32_t gather_workgroups;   /* frames from the host: workgroups of k_gather_frames (rule: 2 per image in the gated layout of a batch, else 32) */
  int32_t klt_reuse;           /* plain tracker, read per launch: 1 = k_klt_track_r (keeps the target window while LK stays in one pixel cell; same bits), -1 = k_klt_track; 0: the rule (k_klt_track_r, unless klt_waves or klt_pair name k_klt_track) */
  int32_t reserved[12];
} vo_tuning;
int32_t vo_get_tuning(vo_ctx* ctx, vo_tuning* out);
int32_t vo_set_tuning(vo_ctx* ctx, const vo_tuning* t);

/* ---- fused per-frame step on resident data ---------------------------------------------------
 * One call enqueues the hot path of one frame in the order of Pipeline.step (src/pipeline/pipeline.py:92-167):
 * frame `frame_idx` of the uploaded sequence -> pyramid/Scharr -> KLT of the resident points -> [DLT of the
 * uploaded pairs] -> [BA of the uploaded problem] -> [Shi-Tomasi re-detection around the tracked points] ->
 * result copies.  With vo_set_graph_mode(ctx, 1) the launch sequence is captured once per buffer parity and replayed
 * as a hipGraph (bit-identical results; off by default: on ROCm 7.2 the replay costs more than ~45 plain launches).
 * Up to TWO steps may be in flight (in graph mode too: a capture is keyed by the mirror half it bakes in): step t + 1 can be enqueued before step t is fetched, the
 * results of consecutive steps land in alternating pinned mirrors, so the GPU queue never drains while the host
 * unpacks.  vo_frame_fetch waits for the OLDEST step not fetched yet (an event, not the whole stream) and unpacks it;
 * with nothing in flight it returns the last step's results again. */
int32_t vo_frame_step_resident(vo_ctx* ctx, int32_t frame_idx, int32_t n_pts, int32_t do_dlt, int32_t do_ba,
                               int32_t do_st, int32_t mask_radius, const vo_klt_params* klt,
                               const vo_st_params* st, const vo_ba_params* ba);               /* async */
int32_t vo_frame_fetch(vo_ctx* ctx, int32_t n_pts, float* p, uint8_t* status, float* err, float* X4,
                       double* depth1, double* reproj, double* poses, double* points, vo_ba_stats* stats,
                       float* corners, int32_t* n_corners);
/* The same step with the frames handed over BY THE HOST, as the reference's loop does (Loader.next -> Pipeline.step(img): src/loader/loader.py:86,
 * src/pipeline/pipeline.py:98,171-172): frames[b] = this step's image of sequence b, `height` rows of `stride` bytes (>= width), uint8.  The
 * upload runs on a copy stream of its own into a device buffer double-buffered by step parity, the pyramid of the step waits for it by an event:
 * with two steps in flight the upload of frame t + 1 overlaps the bundle adjustment of frame t.  Images that follow each other in host memory (a
 * [batch][height][width] array) travel as one copy.  Pinned memory (vo_host_alloc, or registered by the caller) is read by the GPU while the
 * step runs; pageable memory is staged by the runtime (slower).  In flight: up to 2 steps, as vo_frame_step_resident.  Every image a step was
 * given, of any memory kind, must stay allocated and untouched until vo_frame_fetch has returned that step (when a pageable source has been
 * read is up to the runtime, not promised here).  Results are bit-identical to vo_frame_step_resident on the same frames.  Plain launches (a
 * captured graph bakes its source in). */
int32_t vo_frame_step_host(vo_ctx* ctx, const uint8_t* const* frames, int32_t stride, int32_t n_pts, int32_t do_dlt, int32_t do_ba,
                           int32_t do_st, int32_t mask_radius, const vo_klt_params* klt,
                           const vo_st_params* st, const vo_ba_params* ba);                    /* async */
/* page-locked host memory for frames a loader decodes into (numpy arrays over it: VoContext.host_alloc) */
int32_t vo_host_alloc(uint64_t bytes, void** out);
int32_t vo_host_free(void* p);
int32_t vo_set_graph_mode(vo_ctx* ctx, int32_t on);
/* Stream layout of vo_frame_step_resident.  0: one stream.  1 (default): re-detection +
 * triangulation on a side stream beside the bundle adjustment (+10-20 % for one context, +1-2 % with three).  2: pipelined, three
 * streams -- pyramid + KLT | re-detection + triangulation | bundle adjustment -- so that the bundle adjustment of frame t also runs
 * beside the front end of frame t + 1 when two steps are in flight (ONE sequence: 3 600 -> 4 500 frames/s; three batched contexts lose
 * 2 %).  Results are identical in every layout.  Fetch the steps in flight first.
 * Layout 2 with a batch of >= 8 sequences: the tracker's launch (one wave per keypoint, 512 000 workgroups at a batch of 256) takes every free
 * wave slot for its whole duration and the previous frame's LM chain would stand still beside it, so (a) the tracker of frame t + 1 is
 * enqueued behind the first `gate_groups` LM launch groups of frame t -- the groups in which (nearly) all problems still run get the whole
 * chip -- and (b) the ctx stream is re-created as a queue that leaves `reserved_cus` compute units free (one per shader engine and XCD), on
 * which the chain's narrow tail groups run beside the tracker.  +4 % at 256 sequences, +10-14 % at 8-192; a longer LM budget costs (almost)
 * nothing more.  vo_step_layout reports what is in effect; vo_tuning.gate_groups / reserve_cus force other values.  Graph
 * replay and vo_pipe_step run on the plain, unmasked stream. */
int32_t vo_set_side_stream(vo_ctx* ctx, int32_t on);
int32_t vo_step_layout(vo_ctx* ctx, int32_t* layout, int32_t* gate_groups, int32_t* reserved_cus);

/* ---- in-stream timing (hipEvent pairs recorded on the ctx stream around a region's launches) -----
 * Used by bench.py for the roofline figure: region VO_PROF_KLT brackets exactly the k_klt_track launch.
 * vo_profile_read synchronises the stream and returns the summed elapsed time and the number of
 * recorded regions since vo_profile_enable(ctx, mask); mask = OR of (1 << region), 0 = off.
 * VO_PROF_CLAHE_LUT / VO_PROF_CLAHE_APPLY bracket the k_clahe_lut / k_clahe_apply launch of a pyramid build (inside its VO_PROF_FRAME bracket).
 * VO_PROF_HOM_SOLVE / _SCORE / _SELECT / _FINISH bracket the k_h4_solve / k_h4_score / k_h4_select launch of every round of
 * vo_homography_ransac and its k_h4_finish launch (tools/homography_timing.py).
 * VO_PROF_ORB_PYRAMID / _CANDIDATES / _RETAIN / _DESCRIBE bracket the stages of vo_orb_detect_compute: the k_orb_resize launches; k_orb_score,
 * k_orb_nms and k_orb_cut; k_orb_harris and k_orb_rank; k_orb_describe (tools/orb_timing.py).
 * VO_PROF_FUND_SOLVE / _SCORE / _SELECT / _FINISH bracket the k_f7_solve / k_f7_score / k_f7_select launch of every round of
 * vo_fundamental_ransac and its k_f7_finish launch (tools/fundamental_timing.py).
 * VO_PROF_GMATCH_FORWARD / _REVERSE / _ACCEPT bracket the forward pass, the cross-check's reverse pass and the k_match_accept launch of
 * vo_match_guided_hamming / vo_match_guided_l2 (tools/guided_match_timing.py).
 * VO_PROF_HPOSE brackets the k_hpose launch of vo_homography_decompose and vo_homography_pose (tools/hpose_timing.py).
 * VO_PROF_SIM3_SOLVE / _SCORE / _SELECT / _FINISH bracket the k_s3_solve / k_s3_score / k_s3_select launch of every round of
 * vo_sim3_ransac and the k_s3_finish launch of vo_sim3_ransac and vo_sim3_fit (tools/sim3_timing.py).
 * VO_PROF_ALIGN brackets each k_align_level launch of vo_sparse_align, one per level (tools/align_timing.py).
 * VO_PROF_DEPTH brackets the k_depth_update launch of vo_depth_update (tools/depth_timing.py). */
enum { VO_PROF_FRAME = 0, VO_PROF_KLT = 1, VO_PROF_ST = 2, VO_PROF_DLT = 3, VO_PROF_BA = 4, VO_PROF_CLAHE_LUT = 5, VO_PROF_CLAHE_APPLY = 6,
       VO_PROF_HOM_SOLVE = 7, VO_PROF_HOM_SCORE = 8, VO_PROF_HOM_SELECT = 9, VO_PROF_HOM_FINISH = 10, VO_PROF_ORB_PYRAMID = 11,
       VO_PROF_ORB_CANDIDATES = 12, VO_PROF_ORB_RETAIN = 13, VO_PROF_ORB_DESCRIBE = 14,
       VO_PROF_FUND_SOLVE = 15, VO_PROF_FUND_SCORE = 16, VO_PROF_FUND_SELECT = 17, VO_PROF_FUND_FINISH = 18,
       VO_PROF_GMATCH_FORWARD = 19, VO_PROF_GMATCH_REVERSE = 20, VO_PROF_GMATCH_ACCEPT = 21, VO_PROF_HPOSE = 22,
       VO_PROF_SIM3_SOLVE = 23, VO_PROF_SIM3_SCORE = 24, VO_PROF_SIM3_SELECT = 25, VO_PROF_SIM3_FINISH = 26,
       VO_PROF_ALIGN = 27, VO_PROF_DEPTH = 28, VO_PROF_COUNT = 29 };
int32_t vo_profile_enable(vo_ctx* ctx, int32_t region_mask);
int32_t vo_profile_read(vo_ctx* ctx, int32_t region, double* total_ms, int32_t* count);
/* diagnostic: shader-clock stamps (s_memtime deltas, cycles) of the phases of the last launch of a
 * single-workgroup / critical-path kernel.  which: 0 = k_st_select, 1 = k_ba_solve, 2 = k_ba_build (workgroup 0), 3 = k_klt_track (one wave).
 * out8 receives 8 values (unused entries 0).  Synchronises the stream. */
int32_t vo_debug_cycles(vo_ctx* ctx, int32_t which, int64_t* out8);

#ifdef __cplusplus
}
#endif
#endif /* VO_MI355X_H */
