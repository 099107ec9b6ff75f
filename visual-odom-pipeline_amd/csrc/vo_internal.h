// Internal definitions shared by the HIP translation units of libvo_mi355x.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <type_traits>

#include "vo_buf.h"
#include "vo_mi355x.h"

#define VO_PAD 32          // border (pixels) around every pyramid level, >= win + 1
#define VO_MAX_LEVELS 8
#define VO_MAX_WIN 31

struct vo_level {
  int w, h;        // interior size
  int pitch;       // padded row pitch in PIXELS (multiple of 64)
  int ph;          // padded rows = h + 2*VO_PAD
};

struct vo_frame {                // the levels of one frame-store half: plain pointers, owned by vo_ctx::fr_img / fr_der
  uint8_t* img[VO_MAX_LEVELS];   // padded, origin of the interior at (VO_PAD, VO_PAD)
  int16_t* der[VO_MAX_LEVELS];   // padded, interleaved (Ix, Iy), same pixel pitch; border = 0
};

#include <vector>
struct vo_prof {
  int mask = 0;                                                  // bit r = region r is timed
  std::vector<hipEvent_t> pool;                                  // all events ever created (reused)
  size_t used = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pairs[VO_PROF_COUNT];
};

struct vo_st_ws;   // Shi-Tomasi workspace (vo_shi_tomasi.hip)
struct vo_ba_ws;   // bundle-adjustment workspace (vo_ba.hip)

// per-sequence camera data of the two-view triangulation (vo_dlt.hip; written on the device by the closed-loop pipeline)
struct vo_dlt_cam {
  float P0[12], P1[12];    // K @ H[:3,:] rounded to float32, as the reference hands them to cv2.triangulatePoints (extractor.py:268-269)
  double M0[12], M1[12];   // the same products in float64 (filter statistics)
  double H1z[4];           // third row of H1
};

// Rows beside the result slab, one store per opt-in per-point feature (the slab goes to the host whole with every fused frame step: it does not
// grow for a feature that step never runs).  Per sequence up to four typed columns of the same number of rows, in a device allocation of its
// own that is made when the feature is first asked for (a context that never asks has none), and a note of what the last producer left there
struct vo_side_rows {
  vo_dev<uint8_t> d;                 // [batch][seq]; null until reserved
  size_t seq = 0;                    // bytes per sequence
  size_t off[4] = {0, 0, 0, 0};      // column k of sequence 0 starts here
  size_t elem[4] = {0, 0, 0, 0};     // bytes per row of column k
  int n = -1;                        // rows per sequence the last producer wrote, else -1
};
template <class T> inline T* vo_side_col(const vo_side_rows& s, int k) { return reinterpret_cast<T*>(s.d.get() + s.off[k]); }     // column k of sequence 0
struct vo_side_copy { void* h; int col; };     // a host array [batch][n rows] (null = not asked for) and the column it mirrors
enum { VO_FB_P0R, VO_FB_ERR, VO_FB_OK };
enum { VO_SUBPIX_RAW, VO_SUBPIX_OUT, VO_SUBPIX_ITERS, VO_SUBPIX_FLAGS };
enum { VO_BRIEF_DESC, VO_BRIEF_IN, VO_BRIEF_ANGLE, VO_BRIEF_FLAGS };
#define VO_CORNER_CAP 4096          // corners a Shi-Tomasi launch can put out (ST_OUT_CAP)

// A context carries `batch` independent sequences in lockstep: every device buffer has a leading sequence
// dimension with a uniform stride and every kernel a grid dimension over sequences, so that one launch serves
// the whole batch (the path is launch / latency bound per sequence; batching is what fills the 256 CUs).
struct vo_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;     // side stream of the fused frame step: Shi-Tomasi runs beside DLT + BA (fork / join by events)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipStream_t stream3 = nullptr;     // pipelined frame step (vo_set_side_stream(c, 2)): the bundle adjustment of frame t runs here beside the front end of frame t + 1
  hipEvent_t ev_ba[2] = {nullptr, nullptr};     // the BA of the step using half k has published its solution (d_pub)
  hipEvent_t ev_copy1[2] = {nullptr, nullptr};  // the KLT results of the step using half k have left the device (copy on stream A)
  hipEvent_t ev_pub[2] = {nullptr, nullptr};    // ... and the copy of it (on stream2) has left the device: the next k_ba_finalize may overwrite d_pub
  hipEvent_t ev_ba_wide[2] = {nullptr, nullptr}; // pipelined step: the first `ba_wide_groups` LM groups of the step using half k have run (recorded on stream C);
                                                // the NEXT step's tracker launch waits for it -- the wide groups get the whole chip, the tail groups run beside the tracker
  int ba_wide_groups = 0;                       // 0: no gating
  bool ba_wide_recorded = false;
  int stream_reserve = 0;                        // compute units `stream` leaves free (CU mask of its queue; vo_set_side_stream)
  bool layout_suspended = false;                 // vo_pipe_step took the gate and the CU mask off (its chain needs the whole chip): the next frame step re-applies them
  bool pub_copy_pending = false;                // a pipelined step has recorded ev_pub at least once
  // loader pre-filter (vo_set_prefilter): cv2.bilateralFilter taps applied while a frame enters the frame store
  int bil_maxk = 0;                  // 0 = off
  signed char bil_dx[49], bil_dy[49];
  float bil_sw[49];
  vo_dev<float> d_bil_cw;            // [256] colour weights
  int side_stream = 1;               // vo_set_side_stream
  vo_tuning tune = {};               // forced forms (vo_set_tuning); all zero = the library's rules
  bool main_dirty = true;            // an entry point other than vo_pipe_step may have enqueued work on `stream` since the last pipe step (set by
                                     // vo_quiesce_side, which every such entry point calls): the next pipe step orders its side streams behind it
  int batch = 1;
  int width = 0, height = 0, max_pts = 0, max_level = 0, win = 0;
  int top = 0;                       // highest pyramid level index built
  vo_level lv[VO_MAX_LEVELS];
  size_t lvl_px[VO_MAX_LEVELS];      // pixels per sequence per level (= pitch * ph): the per-sequence stride
  vo_frame fr[2] = {};               // sequence 0 of each buffer; sequence b at + b * lvl_px[l] pixels
  vo_dev<uint8_t> fr_img[2][VO_MAX_LEVELS];     // the owners of fr[f].img[l] / der[l]
  vo_dev<int16_t> fr_der[2][VO_MAX_LEVELS];
  int cur = 0;                       // index of the current frame in fr[]
  int n_pushed = 0;
  vo_dev<uint8_t> d_raw;             // staging of one raw frame per sequence
  vo_pinned<uint8_t> h_raw;          // pinned host staging of vo_frame_push (allocated on first use)
  hipEvent_t ev_raw = nullptr;       // the upload out of h_raw is done
  // vo_frame_step_host: the frames of a step arrive from the host on a copy stream of their own, double-buffered like the steps in flight
  hipStream_t stream_h2d = nullptr;
  vo_dev<uint8_t> d_host_raw[2];                    // [batch][h][w], by step parity
  hipEvent_t ev_h2d[2] = {nullptr, nullptr};        // the upload into d_host_raw[k] is complete (recorded on stream_h2d, awaited by the ctx stream)
  hipEvent_t ev_raw_free[2] = {nullptr, nullptr};   // the pyramid has read d_host_raw[k] (recorded on the ctx stream, awaited by stream_h2d)
  bool raw_free_recorded[2] = {false, false};
  int pipe_host_slot = 0;                           // vo_pipe_step_host alternates the two buffers on its own count
  // page-locked [VO_HOST_TAB_SLOTS][batch]: device-visible addresses of a step's images, read by k_gather_frames WHILE it runs -- so one slot per
  // step that can be in flight (vo_host_tab_slot), never one per d_host_raw half
  vo_pinned<const uint8_t*> h_ptr_tab;
  vo_dev<uint8_t> d_seq;             // preloaded sequences [batch][seq_n][h][w] (vo_seq_upload)
  int seq_n = 0;
  // tracked point sets live in the result slab (off_pa / off_pb, ping-pong selected by p_parity)
  int p_parity = 0;                  // 0: current points at off_pa
  vo_dev<int32_t> d_iters;           // [batch][n x (max_level + 1)]
  int n_resident = 0;
  std::vector<float> pts_stage;      // vo_points_in: the caller's point rows with the NaN rows replaced (kept until the upload out of it is done)
  int iters_stride = 0;              // of the last KLT launch
  // The four side-row stores (vo_side_rows; reserved by vo_fb_reserve ... vo_brief_reserve below), M = max_pts, C = max(max_pts, VO_CORNER_CAP):
  //   fb      M rows: p0r 8 B | fb_err 4 B | ok 1 B, every column rounded up to 256 B    n = points of the last track if it ran the check
  //   guess   M rows: the start positions 8 B, in the tracker's point order               n = points of the last track if a predictor wrote them
  //   subpix  C rows: raw 8 | out 8 | iters 4 | flags 1, the sequence rounded up to 16 B  n = corner slots the last resident detection refined
  //   brief   C rows: desc 32 | in 8 | angle 4 | flags 1, the sequence rounded up to 16 B n = corner slots the last resident detection described
  // (subpix out / brief in: the synchronous forms' corner rows; the pipeline's tables never hold a descriptor)
  vo_side_rows fb, guess, subpix, brief;
  float fb_max_err = __builtin_inff();              // forward-backward check (vo_klt_fb.hip): threshold of vo_set_fb_check (+inf = off)
  int klt_predict = VO_KLT_PREDICT_OFF;             // motion-predicted start of the tracker (vo_klt_seed.hip): mode of vo_set_klt_predict
  bool subpix_on = false;                           // sub-pixel corner refinement (vo_subpix.hip): the setting of vo_set_subpix
  vo_subpix_params subpix_prm = {};
  bool brief_on = false;                            // oriented BRIEF (vo_brief.hip): the setting of vo_set_brief with its sampling table (a launch
  vo_brief_params brief_prm = {};                   // takes it by value)
  int8_t brief_pat[1024] = {};
  // lens undistortion (vo_undistort.hip): the setting of vo_set_undistort, its fixed-point map [h][w] of 8-byte entries (shared by the batch)
  // and the tight [batch][h][w] staging image the level-0 kernels read instead of the raw frame -- allocated when first switched on
  bool und_on = false;
  double und_K[4] = {0, 0, 0, 0}, und_dist[8] = {0, 0, 0, 0, 0, 0, 0, 0}, und_newK[4] = {0, 0, 0, 0};
  vo_dev<uint64_t> d_und_tab;
  vo_dev<uint8_t> d_und;
  // CLAHE (vo_clahe.hip): the setting of vo_set_clahe, the tables [batch][tiles_y][tiles_x][256] u8 the last launch wrote (room for 16 x 16
  // tiles) and the tight [batch][h][w] staging image the level-0 kernels read instead of the raw frame -- allocated when first switched on
  bool cl_on = false;
  double cl_clip = 0.0;
  int cl_tx = 0, cl_ty = 0;
  vo_dev<uint8_t> d_clahe_lut;
  vo_dev<uint8_t> d_clahe;
  // bumped by every accepted change of an ingest setting (vo_set_prefilter, vo_set / vo_clear_undistort, vo_set / vo_clear_clahe): all that a
  // captured step's key holds of the ingest chain
  unsigned ingest_gen = 0;
  // DLT inputs
  vo_dev<float> d_uv0, d_uv1;        // [batch][max_pts][2]
  vo_dev<vo_dlt_cam> d_dlt_cam;      // [batch]
  int dlt_n = 0, dlt_stats = 0;
  vo_st_ws* st = nullptr;
  struct vo_pnp_ws* pnp = nullptr;   // PnP-RANSAC workspace (vo_pnp.hip)
  struct vo_sift_ws* sift = nullptr;     // SIFT scale space and lists (vo_sift.hip)
  struct vo_orb_ws* orb = nullptr;       // ORB pyramid, score maps and lists (vo_orb.hip), made by the first vo_orb_detect_compute
  struct vo_match_ws* match = nullptr;   // descriptor matcher buffers, plain and guided (vo_match.hip)
  struct vo_ess_ws* ess = nullptr;   // essential-matrix RANSAC workspace (vo_essential.hip)
  struct vo_hom_ws* hom = nullptr;   // homography RANSAC workspace (vo_homography.hip)
  struct vo_fund_ws* fund = nullptr; // fundamental-matrix RANSAC workspace (vo_fundamental.hip)
  struct vo_hpose_ws* hpose = nullptr; // pose-from-homography workspace (vo_hpose.hip)
  struct vo_sim3_ws* sim3 = nullptr; // Sim(3) / rigid 3D-3D alignment workspace (vo_sim3.hip)
  struct vo_align_ws* align = nullptr; // sparse image alignment workspace (vo_align.hip)
  struct vo_depth_ws* depth = nullptr; // depth filter workspace (vo_depth.hip)
  struct vo_trk_ws* trk = nullptr;   // device-resident track table (vo_tracks.hip)
  struct vo_pipe_ws* pipe = nullptr; // closed-loop Pipeline.step on the device (vo_pipeline.hip)
  const int32_t* d_pt_counts = nullptr;   // vo_tracks_* only (set by vo_tracks_seed, cleared by vo_trk_destroy): per-sequence number of live tracks the
                                          // PUBLIC resident entry points (vo_klt_track_resident, vo_shi_tomasi_resident) then use; null = uniform n.
                                          // The closed-loop pipeline passes its own counters explicitly (the resident enqueues) and never touches this.
  vo_ba_ws* ba = nullptr;
  vo_prof prof;
  vo_dev<unsigned long long> d_dbg;      // 4 x 8 phase stamps (vo_debug_cycles)
  // result slab: every per-frame output of the front end lives in ONE device allocation (mirrored in pinned host
  // memory) so that a frame's results come back with a single D2H copy instead of ten.
  vo_dev<uint8_t> d_slab;                // [batch][slab_seq]
  vo_pinned<uint8_t> h_slab;             // pinned, 2 x slab_bytes: steps alternate between the halves so that step t + 1 can
                                         // be enqueued while the host still reads step t (vo_frame_step_resident / vo_frame_fetch)
  hipEvent_t ev_step[2] = {nullptr, nullptr};   // recorded after the result copies of the step using half k
  size_t step_off_p[2] = {0, 0};         // slab offset of the tracked points of that step
  long steps_enq = 0, steps_fetched = 0;
  size_t slab_seq = 0;                   // bytes per sequence
  size_t slab_bytes = 0;                 // batch * slab_seq
  size_t off_pa = 0, off_pb = 0, off_status = 0, off_err = 0, off_X4 = 0, off_depth = 0, off_reproj = 0,
         off_st_scalars = 0, off_st_out = 0;
  // per-frame step (vo_frame_step_resident) captured as hipGraphs, one per frame parity
  // captured steps, keyed by the hash of everything a capture bakes in: parameters by value, device pointers (the selected problem of a
  // BA bank among them), problem shapes, frame-store parity and the pinned mirror half the results go to
  std::vector<std::pair<uint64_t, hipGraphExec_t>> step_graphs;
  vo_dev<int32_t> d_frame_idx;           // frame index consumed by the captured k_pad_level0
  vo_pinned<int32_t> h_frame_idx;        // pinned ring of frame indices (H2D source must outlive the copy)
  int frame_ring = 0;
  int use_graph = 0;                     // hipGraph replay is opt-in (vo_set_graph_mode): on ROCm 7.2 it is slower than plain launches
  // landmark-sharded bundle adjustment (vo_comm.hip): RCCL communicator of this context, one process per GPU
  void* comm = nullptr;                  // ncclComm_t
  int comm_rank = 0, comm_ranks = 1;
  int ba_sharded = 0;                    // batch entries (and ranks) are landmark shards of ONE problem
  std::string err;
};

inline int32_t vo_fail(vo_ctx* c, int32_t code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

#define VO_HIP(c, expr)                                                                   \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess) {                                                               \
      char _b[512];                                                                       \
      snprintf(_b, sizeof(_b), "%s:%d: %s -> %s", __FILE__, __LINE__, #expr,              \
               hipGetErrorString(_e));                                                    \
      return vo_fail((c), VO_E_HIP, _b);                                                  \
    }                                                                                     \
  } while (0)

// (VO_CHECK_AS: in a body several entry points share, under the entry's name `who`)
#define VO_CHECK_AS(c, who, cond, code, msg)                                              \
  do {                                                                                    \
    if (!(cond)) return vo_fail((c), (code), std::string(who) + ": " + (msg));            \
  } while (0)
#define VO_CHECK(c, cond, code, msg) VO_CHECK_AS(c, __func__, cond, code, msg)

// slab accessors (sequence 0; sequence b at + b * slab_seq bytes)
template <class T> inline T* vo_slab(const vo_ctx* c, size_t off) { return reinterpret_cast<T*>(c->d_slab.get() + off); }
inline size_t vo_off_p(const vo_ctx* c) { return c->p_parity ? c->off_pb : c->off_pa; }       // current points
inline size_t vo_off_p_next(const vo_ctx* c) { return c->p_parity ? c->off_pa : c->off_pb; }  // KLT output
// device side: pointer of sequence b given the sequence-0 pointer and the byte stride
template <class T> __device__ __forceinline__ T* vo_seq(T* base, size_t stride_bytes, int b) {
  return reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(const_cast<typename std::remove_const<T>::type*>(base)) + (size_t)b * stride_bytes);
}

// XCD-aware (block, sequence) assignment for grids of `nblk` blocks per sequence x `batch` sequences, batch % 8 == 0:
// workgroups are dealt to the 8 XCDs round-robin in dispatch order and every XCD has its own L2, so with the plain mapping the
// neighbouring blocks of one image land on eight different L2s and each fetches the rows they share.  Remapped, XCD k works on
// sequences k, k + 8, ... one after the other: a sequence's rows are fetched by ONE L2, and what one kernel of the frame chain
// wrote there (plain stores keep the line) the next kernel finds there.  Placement is an observation, not a contract: the
// mapping is a bijection of the grid, so results never depend on it.  id = linear block index in dispatch order.
__device__ __forceinline__ void vo_xcd_assign(unsigned id, unsigned nblk, int remap, int& blk, int& bseq) {
  if (remap) {
    const unsigned q = id >> 3;
    bseq = (int)(id & 7u) + 8 * (int)(q / nblk);
    blk = (int)(q % nblk);
  } else {
    bseq = (int)(id / nblk);
    blk = (int)(id - (unsigned)bseq * nblk);
  }
}

// RAII bracket: records an event pair on stream q around a region when profiling is on
struct vo_prof_scope {
  vo_ctx* c; hipStream_t q; int region; hipEvent_t e0 = nullptr, e1 = nullptr;
  vo_prof_scope(vo_ctx* c_, hipStream_t q_, int region_);
  ~vo_prof_scope();
};

// phase stamp helper for the diagnostic cycle counters (thread 0 of a workgroup)
#define VO_STAMP(buf, idx) do { if ((buf) && threadIdx.x == 0) (buf)[idx] = __builtin_amdgcn_s_memtime(); } while (0)

static inline int vo_div_up(int a, int b) { return (a + b - 1) / b; }

// waits for every stream a frame step enqueues on: the ctx stream, then the side streams where they exist
inline int32_t vo_sync_streams(vo_ctx* c) {
  VO_HIP(c, hipStreamSynchronize(c->stream));
  if (c->stream2) VO_HIP(c, hipStreamSynchronize(c->stream2));
  if (c->stream3) VO_HIP(c, hipStreamSynchronize(c->stream3));
  return VO_OK;
}

// Stream fork and join of the two step orchestrators (step_enqueue, vo_step.hip; pipe_step, vo_pipeline.hip); after a call that failed nothing
// further is issued.  fork: `ev` recorded on `from`; `to` waits for it, and `to2` (null = there is none: the library forks to streams it made)
inline hipError_t vo_stream_fork(hipEvent_t ev, hipStream_t from, hipStream_t to, hipStream_t to2 = nullptr) {
  hipError_t e = hipEventRecord(ev, from);
  if (e == hipSuccess) e = hipStreamWaitEvent(to, ev, 0);
  if (e == hipSuccess && to2) e = hipStreamWaitEvent(to2, ev, 0);
  return e;
}
// join: `ev` recorded on `side`, `main` waits for it.  Every exit behind a fork joins: work queued on the side stream stays ordered before what the
// caller enqueues (or frees) next on the main stream, also when a later enqueue fails -- a caller on a failing path joins, then returns its own code
inline hipError_t vo_stream_join(hipEvent_t ev, hipStream_t side, hipStream_t main) {
  const hipError_t e = hipEventRecord(ev, side);
  return e == hipSuccess ? hipStreamWaitEvent(main, ev, 0) : e;
}

// cross-unit internals used by the fused frame step (vo_step.hip).  Every function that enqueues takes the stream q its launches, copies, event
// records and profile brackets go to, and never waits for the side streams: that (vo_quiesce_side) is the extern "C" entry points' business
int32_t vo_build_pyramid(vo_ctx* c, hipStream_t q, const uint8_t* d_raw_img, size_t raw_seq_stride, const int32_t* d_frame_idx);
// Where a step's frame comes from: sequence 0's image, the bytes to the next sequence's, the frame index on the device (a captured step: `raw` is then the
// sequence store) or null, the d_host_raw half of an upload (-1: resident).  vo_frame_src_pyramid on q: waits for ev_h2d[half], builds the pyramid, records ev_raw_free[half]
struct vo_frame_src { const uint8_t* raw; size_t seq_stride; const int32_t* d_frame_idx; int host_half; };
inline vo_frame_src vo_frame_src_host(const vo_ctx* c, int half) { return {c->d_host_raw[half], (size_t)c->width * c->height, nullptr, half}; }
inline vo_frame_src vo_frame_src_resident(const vo_ctx* c, int frame_idx, const int32_t* d_frame_idx) {
  return {c->d_seq + (d_frame_idx ? 0 : (size_t)frame_idx * c->width * c->height), (size_t)c->width * c->height * c->seq_n, d_frame_idx, -1};
}
int32_t vo_frame_src_pyramid(vo_ctx* c, hipStream_t q, const vo_frame_src& s);
// what the two *_step_host entries share.  vo_host_frames_admit: `frames`, `stride` and every frames[b], VO_E_INVALID under the entry's name `who`;
// vo_host_frames_abandon: (error path) the step does not count, so its pointer-table row goes to the next one: let the gather finish reading it
int32_t vo_host_frames_admit(vo_ctx* c, const char* who, const uint8_t* const* frames, int32_t stride);
inline void vo_host_frames_abandon(vo_ctx* c) { (void)hipStreamSynchronize(c->stream_h2d); }
// a step's `batch` images from the host into d_host_raw[slot] on the copy stream (vo_step.hip); ev_h2d[slot] is recorded behind it
// tab_slot: the row of h_ptr_tab this step's pointers go to (vo_host_tab_slot_frame / vo_host_tab_slot_pipe)
int32_t vo_host_frames_upload(vo_ctx* c, const uint8_t* const* frames, int32_t stride, int slot, int tab_slot);
// The pointer table's rows: [0, 2) the frame step (vo_frame_step_host admits 2 in flight), by steps_enq & 1; [2, 2 + VO_PIPE_INFLIGHT) the closed
// loop (vo_pipe_step_host admits VO_PIPE_INFLIGHT), by pipe->enq % VO_PIPE_INFLIGHT.  A row is written again only once the step that used it
// has been fetched, and a fetched step's gather is done (its pyramid waited for ev_h2d before it ran).  The two paths never share a row.
#define VO_HOST_TAB_SLOTS (2 + VO_PIPE_INFLIGHT)
inline int vo_host_tab_slot_frame(long steps_enq) { return (int)(steps_enq & 1); }
inline int vo_host_tab_slot_pipe(long pipe_enq) { return 2 + (int)(pipe_enq % VO_PIPE_INFLIGHT); }
int32_t vo_ba_enqueue_pub_copy(vo_ctx* c, hipStream_t q, int half);     // half: which pinned mirror (0 / 1)
void vo_ba_unpack_pub(vo_ctx* c, int half, double* poses_out, double* points_out, vo_ba_stats* stats);   // arrays over the batch
bool vo_ba_ready(const vo_ctx* c);
double* vo_ba_obs_device(vo_ctx* c, int* n_slots, int* n_pts);   // resident observation table [batch][W][N][2] of the uploaded problem
bool vo_st_ready(const vo_ctx* c);
int vo_st_last_max_corners(const vo_ctx* c);
int vo_st_launch_state(const vo_ctx* c);
int vo_st_flags_save(const vo_ctx* c);
void vo_st_flags_restore(vo_ctx* c, int saved);
// the pipelined stream layout (vo_set_side_stream 2) leaves work on streams B and C after a step: every entry point outside the
// step / fetch pair that touches the result slab, the frame store, the BA / Shi-Tomasi / DLT / PnP workspaces waits for them first
int32_t vo_quiesce_side(vo_ctx* c);
bool vo_blocking_sync();             // environment VO_BLOCKING_SYNC=1: events a host thread waits on sleep in the driver instead of spinning
int32_t vo_main_stream_reserve(vo_ctx* c, int reserve);               // the ctx stream re-created with / without a CU mask (vo_set_side_stream(c, 2) of a batch)
hipError_t vo_stream_create(hipStream_t* st, int reserve_cus);      // reserve_cus > 0: the queue never uses the last `reserve_cus` bits of the CU mask
int32_t vo_st_prepare(vo_ctx* c, const vo_st_params* prm);
// vo_st_params.fast_threshold and what it excludes: VO_OK or VO_E_INVALID (nothing enqueued); the orchestrators ask before their first enqueue
int32_t vo_st_check_params(vo_ctx* c, const vo_st_params* prm);
// a captured step that re-detects is replayed: the host-side notes its st_launch made at capture time (mask state, kept map, corner capacity), made again
void vo_st_note_replay(vo_ctx* c, const vo_st_params* prm);
// FAST-9/16 response (vo_fast.hip) of the current frame's level 0 for st_launch: R [batch][h][w] into d_R (every pixel), the masked maxima of its
// vo_fast_n_blockmax(w, h) workgroups per sequence into d_blockmax
int vo_fast_n_blockmax(int W, int H);
void vo_fast_enqueue(vo_ctx* c, hipStream_t q, int t, const uint8_t* d_mask, float* d_R, float* d_blockmax);
// the resident enqueues with the per-sequence counters named by the caller (device arrays [batch], null = uniform): d_counts = live
// points of each sequence (KLT input / exclusion discs), d_limit = cap on the corners each sequence's re-detection needs
// The tracker's form word: KLT_FORM_FB = with the forward-backward check (the ok flags land in vo_fb_ok(c) [batch][fb.seq bytes]),
// KLT_FORM_SEEDED = started at the guesses a predictor kernel has just written to c->guess on q (vo_guess_reserve: those rows exist
// afterwards).  The four values select k_klt_track, k_klt_track_fb, k_klt_seeded, k_klt_seeded_fb (vo_klt_enqueue, vo_klt.hip).
enum : unsigned { KLT_FORM_FB = 1u, KLT_FORM_SEEDED = 2u };
int32_t vo_klt_track_resident_enqueue(vo_ctx* c, hipStream_t q, int32_t n, const vo_klt_params* prm, const int32_t* d_counts, unsigned form);
inline bool vo_fb_on(const vo_ctx* c) { return !(c->fb_max_err == __builtin_inff()); }     // +inf = off
inline const uint8_t* vo_fb_ok(const vo_ctx* c) { return vo_side_col<const uint8_t>(c->fb, VO_FB_OK); }
inline bool vo_predict_on(const vo_ctx* c) { return c->klt_predict != VO_KLT_PREDICT_OFF; }
// the form the context's settings ask for (vo_set_fb_check, vo_set_klt_predict): what vo_tracks_track and the closed loop's TRACK stage run
inline unsigned vo_klt_form(const vo_ctx* c) { return (vo_fb_on(c) ? KLT_FORM_FB : 0u) | (vo_predict_on(c) ? KLT_FORM_SEEDED : 0u); }
// The corner stages' launches on the corner rows the selection kernel has just left in st_out on q, `cap` slots per sequence against the current
// frame (vo_corners_detected below is their one caller): k_brief_describe writes a descriptor, an angle and a flag per row into c->brief;
// k_corner_subpix refines the rows in place and notes the integer corner, the iterations and a flag per row in c->subpix
int32_t vo_brief_launch_detected(vo_ctx* c, hipStream_t q, int cap);
int32_t vo_subpix_launch_detected(vo_ctx* c, hipStream_t q, int cap);
int32_t vo_brief_check_pattern(vo_ctx* c, const int8_t* pattern);    // a caller's sampling table: VO_OK or VO_E_INVALID; null = the default table
void vo_orb_destroy(vo_ctx* c);                                      // the ORB pyramid and lists (vo_orb.hip)
// The ingest chain (vo_frame.hip): the optional stages vo_build_pyramid runs in front of level 0, in this order: lens undistortion
// (vo_undistort.hip), then CLAHE (vo_clahe.hip).  A stage's enqueue takes the frames (k_pad_level0's triple) to its own tight [batch][h][w]
// staging image on q; the next stage, and at last the level-0 kernel, read that image as their raw frame.
typedef void (*vo_ingest_enqueue_fn)(vo_ctx* c, hipStream_t q, const uint8_t* d_raw_img, size_t raw_seq_stride, const int32_t* d_frame_idx, int remap);
struct vo_ingest_stage { bool on; vo_ingest_enqueue_fn enqueue; uint8_t* staging; };
void vo_undistort_enqueue(vo_ctx* c, hipStream_t q, const uint8_t* d_raw_img, size_t raw_seq_stride, const int32_t* d_frame_idx, int remap);
void vo_clahe_enqueue(vo_ctx* c, hipStream_t q, const uint8_t* d_raw_img, size_t raw_seq_stride, const int32_t* d_frame_idx, int remap);
// what the stages' entry points share.  A setting change: vo_ingest_reserve (the staging image, if absent), vo_sync_streams (no build in flight
// runs with the setting that is replaced), the caller's upload or reset on the ctx stream, vo_ingest_commit (waits for it, switches the stage
// on, bumps ingest_gen), then the caller's fields.  vo_ingest_run: a stage alone on `batch` host images, [batch][height] rows of `stride` (in) /
// width (out) bytes; VO_E_STATE with `off_msg` when the stage is off.  vo_ingest_free: the stage is off (vo_ctx_destroy, which releases its buffers)
int32_t vo_ingest_reserve(vo_ctx* c, vo_dev<uint8_t>* staging);
int32_t vo_ingest_commit(vo_ctx* c, bool* on);
int32_t vo_ingest_run(vo_ctx* c, const vo_ingest_stage& s, const char* off_msg, const uint8_t* img, int32_t stride, uint8_t* out);
void vo_ingest_free(bool* on);
int32_t vo_shi_tomasi_resident_counts(vo_ctx* c, hipStream_t q, int32_t n_cur, int32_t mask_radius, const vo_st_params* prm, const int32_t* d_counts,
                                      const int32_t* d_limit);

// collectives on stream q (vo_comm.hip); identity / device copy without a communicator
int32_t vo_comm_allreduce_f64(vo_ctx* c, hipStream_t q, double* buf, size_t count);
int32_t vo_comm_allgather_f64(vo_ctx* c, hipStream_t q, const double* send, double* recv, size_t count);

void vo_trk_destroy(vo_ctx* c);
void vo_pipe_destroy(vo_ctx* c);
bool vo_pipe_busy(const vo_ctx* c);            // closed-loop steps enqueued and not fetched yet

// ---- hooks of the closed-loop pipeline (vo_pipeline.hip) into the stage units: device-resident inputs, per-sequence counts ----
// bundle adjustment: workspace for W slots x N landmark slots with K uploaded, problem written on the device into x0 / obs
// LM state of one bundle-adjustment problem; also the header of the publish buffer [ba_state, padded to VO_BA_PUB_HEADER bytes | x] that
// k_ba_finalize writes and vo_ba_fetch / k_pipe_writeback read
struct ba_state {
  double lambda, nu, cost, cost0;
  int cur, iter, accepted, status, done, n_obs;
};
#define VO_BA_PUB_HEADER 64
static_assert(sizeof(ba_state) <= VO_BA_PUB_HEADER, "the publish buffer's header holds one ba_state");
struct vo_ba_view { double* x0; double* obs; const uint8_t* pub; size_t pub_bytes; size_t x_stride; size_t obs_stride; int W, N; };
int32_t vo_ba_reserve(vo_ctx* c, const double* K_host, int W, int N);
int32_t vo_ba_get_view(vo_ctx* c, vo_ba_view* v);
int32_t vo_ba_check_params(vo_ctx* c, const vo_ba_params* prm);   // loss code and f_scale: VO_OK or VO_E_INVALID (nothing enqueued)
// what one enqueue of the bundle adjustment is told beside its parameters; all zero = none of it
struct vo_ba_enqueue_opts {
  hipEvent_t wait_before_publish;   // k_ba_finalize waits for it (pipelined frame step: the copy of the previous solution has left d_pub)
  hipEvent_t wide_event;            // recorded behind the first `wide_groups` LM groups (pipelined frame step: the next tracker launch waits for it)
  int wide_groups;
  const int32_t* d_live;            // closed loop: d_live[b * live_stride] landmark slots of problem b are in use (device counters); null = all N
  int live_stride;
};
int32_t vo_ba_enqueue_solve(vo_ctx* c, hipStream_t q, const vo_ba_params* prm, const vo_ba_enqueue_opts& o);   // vo_ba_solve_resident's enqueue
int32_t vo_ba_enqueue_budget(vo_ctx* c, hipStream_t q, const vo_ba_params* prm, int it0, int n_it, const vo_ba_enqueue_opts& o);   // iterations it0 .. it0 + n_it - 1, then publish
// 3D-2D pose: correspondences written on the device, counts[b] of them per sequence
struct vo_pnp_view { float* X; float* uv; const uint8_t* mask; const double* out; const int32_t* ctrl; size_t ctrl_stride; int cap; };
int32_t vo_pnp_reserve(vo_ctx* c, const double* K_host);
int32_t vo_pnp_get_view(vo_ctx* c, vo_pnp_view* v);
int32_t vo_pnp_enqueue_counts(vo_ctx* c, hipStream_t q, const vo_pnp_params* prm, int blind_batches, const int32_t* d_counts);
// triangulation of up to n_hi pairs per sequence (c->d_uv0 / d_uv1), counts[b] valid; point i of sequence b uses cams[b][cam_sel[b][i]]
int32_t vo_dlt_enqueue_counts(vo_ctx* c, hipStream_t q, int n_hi, const int32_t* d_counts, const vo_dlt_cam* d_cams, const int32_t* d_cam_sel, int cams_per_seq);
int32_t vo_dlt_enqueue(vo_ctx* c, hipStream_t q, int n);     // the uploaded pairs (vo_dlt_resident's enqueue), n = c->dlt_n > 0: the caller's check
void vo_pnp_destroy(vo_ctx* c);
void vo_ess_destroy(vo_ctx* c);
void vo_hom_destroy(vo_ctx* c);
void vo_fund_destroy(vo_ctx* c);
void vo_hpose_destroy(vo_ctx* c);
void vo_sim3_destroy(vo_ctx* c);
void vo_align_destroy(vo_ctx* c);
void vo_depth_destroy(vo_ctx* c);
// vo_homography_ransac with work enqueued behind k_h4_finish on the same stream, in front of the one read-back (vo_homography_pose):
// `enqueue` gets the search's device buffers -- points [batch][2][cap][2], the refined H of sequence b at d_H + b * h_stride (NaN
// without a model), the winner's mask [batch][cap] -- and what it copies to pinned memory on q is complete when the call returns
struct vo_hom_tail {
  int32_t (*enqueue)(vo_ctx* c, hipStream_t q, const float* d_p, int cap, int n, const double* d_H, int h_stride, const uint8_t* d_mask, void* user);
  void* user;
};
int32_t vo_hom_ransac_tail(vo_ctx* c, const float* pts1, const float* pts2, int32_t n, const vo_hom_params* prm, double* H, double* H0,
                           uint8_t* inlier_mask, vo_hom_stats* stats, const vo_hom_tail* tail);
void vo_match_destroy(vo_ctx* c);
void vo_sift_destroy(vo_ctx* c);
// sub-workspace lifetime hooks
void vo_st_destroy(vo_ctx* c);
void vo_ba_destroy(vo_ctx* c);

// strided copies on the ctx stream between [batch][row_bytes] host arrays and per-sequence device rows d_stride bytes apart
inline hipError_t rows_h2d(vo_ctx* c, void* d, size_t d_stride, const void* h, size_t row_bytes) {
  return hipMemcpy2DAsync(d, d_stride, h, row_bytes, row_bytes, c->batch, hipMemcpyHostToDevice, c->stream);
}
inline hipError_t rows_d2h(vo_ctx* c, void* h, const void* d, size_t d_stride, size_t row_bytes) {
  return hipMemcpy2DAsync(h, row_bytes, d, d_stride, row_bytes, c->batch, hipMemcpyDeviceToHost, c->stream);
}

// Front-end contract (vo_mi355x.h): a caller's point row with a NaN component enters the device as (+inf, +inf).  OpenCV's cvFloor makes
// INT_MIN of a NaN (outside every level: status 0, err 0, no level entered, p1 not finite), while the tracker's saturating conversion makes 0 of
// it and would track the image origin; +inf saturates to INT_MAX and is outside every level there too.  -> h itself when no row has a NaN
// (the usual case: one pass over the floats), else a copy in c->pts_stage, which must stay untouched until the upload out of it has completed
inline bool vo_row_has_nan(const float* row) { return row[0] != row[0] || row[1] != row[1]; }
inline const float* vo_points_in(vo_ctx* c, const float* h, size_t n_rows) {
  size_t i = 0;
  while (i < n_rows && !vo_row_has_nan(h + 2 * i)) i++;
  if (i == n_rows) return h;
  c->pts_stage.assign(h, h + 2 * n_rows);
  for (; i < n_rows; i++)
    if (vo_row_has_nan(h + 2 * i)) c->pts_stage[2 * i] = c->pts_stage[2 * i + 1] = __builtin_inff();
  return c->pts_stage.data();
}

// ---- the side-row stores (vo_side_rows; the four layouts: at the members of vo_ctx) ----
// columns of `cap` rows of elem[k] bytes, each column rounded up to col_align bytes and the sequence to seq_align (1 = as it comes)
inline void vo_side_layout(vo_side_rows* s, int cap, std::initializer_list<size_t> elem, size_t col_align, size_t seq_align) {
  size_t at = 0;
  int k = 0;
  for (size_t e : elem) {
    s->off[k] = at; s->elem[k++] = e;
    at += (e * (size_t)cap + col_align - 1) / col_align * col_align;
  }
  s->seq = (at + seq_align - 1) / seq_align * seq_align;
}
// the allocation, if absent; a refused one leaves the store as it was (not reserved, no layout)
inline int32_t vo_side_reserve(vo_ctx* c, vo_side_rows* s, int cap, std::initializer_list<size_t> elem, size_t col_align, size_t seq_align) {
  if (s->d) return VO_OK;
  vo_side_rows t;
  t.n = s->n;
  vo_side_layout(&t, cap, elem, col_align, seq_align);
  VO_HIP(c, t.d.reserve(t.seq * (size_t)c->batch));
  *s = std::move(t);
  return VO_OK;
}
inline void vo_side_free(vo_side_rows* s) { s->d.reset(); }
inline int vo_corner_cap(const vo_ctx* c) { return c->max_pts > VO_CORNER_CAP ? c->max_pts : VO_CORNER_CAP; }
inline int32_t vo_fb_reserve(vo_ctx* c) { return vo_side_reserve(c, &c->fb, c->max_pts, {8, 4, 1}, 256, 1); }
inline int32_t vo_guess_reserve(vo_ctx* c) { return vo_side_reserve(c, &c->guess, c->max_pts, {8}, 1, 1); }
inline int32_t vo_subpix_reserve(vo_ctx* c) { return vo_side_reserve(c, &c->subpix, vo_corner_cap(c), {8, 8, 4, 1}, 1, 16); }
inline int32_t vo_brief_reserve(vo_ctx* c) { return vo_side_reserve(c, &c->brief, vo_corner_cap(c), {32, 8, 4, 1}, 1, 16); }
// a setter that switches its feature on: the rows exist before the first enqueue that needs them
inline int32_t vo_side_reserve_on_device(vo_ctx* c, int32_t (*reserve)(vo_ctx*)) {
  VO_HIP(c, hipSetDevice(c->device));
  return reserve(c);
}
// n rows of column k of every sequence <-> a host array [batch][n rows], on the ctx stream
inline hipError_t vo_side_h2d(vo_ctx* c, const vo_side_rows& s, int k, const void* h, int n) {
  return rows_h2d(c, vo_side_col<uint8_t>(s, k), s.seq, h, s.elem[k] * (size_t)n);
}
inline hipError_t vo_side_d2h(vo_ctx* c, const vo_side_rows& s, int k, void* h, int n) {
  return rows_d2h(c, h, vo_side_col<const uint8_t>(s, k), s.seq, s.elem[k] * (size_t)n);
}
// the read-backs of n rows into the host arrays that were asked for, in the order named, then the one wait for the ctx stream
inline int32_t vo_side_fetch(vo_ctx* c, const vo_side_rows& s, int32_t n, std::initializer_list<vo_side_copy> cols) {
  if (n > 0)
    for (const vo_side_copy& k : cols)
      if (k.h) VO_HIP(c, vo_side_d2h(c, s, k.col, k.h, n));
  VO_HIP(c, hipStreamSynchronize(c->stream));
  return VO_OK;
}
// The one body of vo_fb_read, vo_klt_guess_read, vo_subpix_read and vo_brief_read, under the export's name `who`: no steps in flight, the last
// producer wrote (else VO_E_STATE with `not_written`), n within what it wrote (else VO_E_INVALID with `n_exceeds`); then the side streams
// are waited for and the columns come back.  need_all: with n > 0 a null array is refused (behind the wait, where vo_klt_guess_read refuses it)
inline int32_t vo_side_read(vo_ctx* c, const char* who, const vo_side_rows& s, const char* not_written, const char* n_exceeds, int32_t n,
                            std::initializer_list<vo_side_copy> cols, bool need_all = false) {
  VO_CHECK_AS(c, who, !vo_pipe_busy(c) && c->steps_enq == c->steps_fetched, VO_E_STATE, "steps in flight: fetch them first");
  VO_CHECK_AS(c, who, s.n >= 0, VO_E_STATE, not_written);
  VO_CHECK_AS(c, who, n >= 0 && n <= s.n, VO_E_INVALID, n_exceeds);
  VO_HIP(c, hipSetDevice(c->device));
  { const int32_t rq = vo_quiesce_side(c); if (rq != VO_OK) return rq; }
  if (need_all && n > 0)
    for (const vo_side_copy& k : cols) VO_CHECK_AS(c, who, k.h, VO_E_INVALID, "null buffer");
  return vo_side_fetch(c, s, n, cols);
}

// ---- the two corner stages (vo_subpix.hip, vo_brief.hip): both work on corner rows [n][2] f32 and keep a vo_side_rows store ----
// The synchronous forms (vo_corner_subpix, vo_brief_compute) behind their null-context check and default parameters, under the export's name
// `who`: `which`, n, the unit's own parameter rules (unit_check), the frame store; n = 0 ends there.  Then `corners` go up into column in_col of
// the reserved store, launch(frame) enqueues the unit's kernel on the ctx stream over those rows, and `outs` come back (the first is required)
template <class Check, class Launch>
int32_t vo_corner_sync(vo_ctx* c, const char* who, vo_side_rows* s, int32_t (*reserve)(vo_ctx*), int in_col, int32_t which, const float* corners,
                       int32_t n, Check unit_check, Launch launch, std::initializer_list<vo_side_copy> outs) {
  VO_CHECK_AS(c, who, which == 0 || which == 1, VO_E_INVALID, "which must be 0 (previous frame) or 1 (current frame)");
  VO_CHECK_AS(c, who, n >= 0 && n <= c->max_pts, VO_E_INVALID, "n exceeds max_pts");
  { const int32_t r = unit_check(); if (r != VO_OK) return r; }
  VO_CHECK_AS(c, who, c->n_pushed >= (which == 0 ? 2 : 1), VO_E_STATE, "frame not pushed yet");
  if (n == 0) return VO_OK;
  VO_CHECK_AS(c, who, corners && outs.begin()->h, VO_E_INVALID, "null buffer");
  VO_HIP(c, hipSetDevice(c->device));
  { const int32_t rq = vo_quiesce_side(c); if (rq != VO_OK) return rq; }
  { const int32_t rr = reserve(c); if (rr != VO_OK) return rr; }
  s->n = -1;                              // the rows no longer describe a detection
  VO_HIP(c, vo_side_h2d(c, *s, in_col, corners, n));
  { const int32_t r = launch(c->fr[which == 1 ? c->cur : (c->cur ^ 1)]); if (r != VO_OK) return r; }
  return vo_side_fetch(c, *s, n, outs);
}
// vo_get_subpix / vo_get_brief: the switch, and the parameters in force (off: the defaults)
template <class P>
int32_t vo_corner_get(vo_ctx* c, bool vo_ctx::*on_m, P vo_ctx::*prm_m, int32_t (*defaults)(P*), int32_t* on, P* prm) {
  if (!c || !on) return VO_E_INVALID;
  *on = c->*on_m ? 1 : 0;
  if (prm) { if (c->*on_m) *prm = c->*prm_m; else defaults(prm); }
  return VO_OK;
}
// one stage behind a resident detection: off, it only notes that the last detection did not run it
inline int32_t vo_corner_stage_detected(vo_ctx* c, hipStream_t q, int max_corners, bool on, vo_side_rows* s, int32_t (*reserve)(vo_ctx*),
                                        int32_t (*launch)(vo_ctx*, hipStream_t, int)) {
  s->n = -1;
  if (!on) return VO_OK;
  { const int32_t rr = reserve(c); if (rr != VO_OK) return rr; }
  const int cap = (max_corners > 0 && max_corners < VO_CORNER_CAP) ? max_corners : VO_CORNER_CAP;
  const int32_t r = launch(c, q, cap);
  if (r != VO_OK) return r;
  s->n = cap;
  return VO_OK;
}
// The hook of every detection that spawns tracks (vo_tracks_detect, the closed loop's DETECT stage), right behind the Shi-Tomasi enqueue on q and
// in front of the spawn: vo_set_brief's descriptors FIRST, so that they always see the integer corners, then vo_set_subpix's refinement, which
// moves the rows of st_out in place
inline int32_t vo_corners_detected(vo_ctx* c, hipStream_t q, int max_corners) {
  const int32_t r = vo_corner_stage_detected(c, q, max_corners, c->brief_on, &c->brief, vo_brief_reserve, vo_brief_launch_detected);
  return r != VO_OK ? r : vo_corner_stage_detected(c, q, max_corners, c->subpix_on, &c->subpix, vo_subpix_reserve, vo_subpix_launch_detected);
}
