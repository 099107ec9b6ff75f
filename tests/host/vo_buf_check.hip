// Stand-alone host check of csrc/vo_buf.h: the owning buffer and the build-then-attach helper against a malloc / free memory policy that
// counts live blocks and refuses the k-th allocation.  No HIP call is made and no device is opened; tests/test_vo_buf.py builds it with
// AddressSanitizer and UBSan, which see a double free, a leak or a use after free that the counts would miss.
#include "vo_buf.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <utility>

static int g_live = 0, g_allocs = 0, g_releases = 0;
static int g_fail_at = -1;        // the allocation (counted from 0 since the last arm()) that is refused; -1: none
static int g_seen = 0;

static void arm(int fail_at) { g_fail_at = fail_at; g_seen = 0; }

// two policies over the same counters, as the library has two over the same runtime
template <int Tag>
struct test_mem {
  static hipError_t alloc(void** p, size_t bytes) {
    if (g_seen++ == g_fail_at) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    if (!*p) return hipErrorOutOfMemory;
    memset(*p, 0xA5, bytes);          // every byte that was asked for is writable
    g_live++; g_allocs++;
    return hipSuccess;
  }
  static void release(void* p) { free(p); g_live--; g_releases++; }
};
template <class T> using t_dev = vo_buf<T, test_mem<0>>;
template <class T> using t_pin = vo_buf<T, test_mem<1>>;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

static void check_reserve() {
  arm(-1);
  t_dev<double> b;
  CHECK(b.get() == nullptr && b.cap() == 0 && b.bytes() == 0 && !b.grew());
  // reserve(0) on an empty buffer allocates nothing
  const int a0 = g_allocs;
  CHECK(b.reserve(0) == hipSuccess);
  CHECK(g_allocs == a0 && b.get() == nullptr && b.cap() == 0 && !b.grew());
  // the first reserve allocates once and releases nothing
  const int r0 = g_releases;
  CHECK(b.reserve(10) == hipSuccess);
  CHECK(g_allocs == a0 + 1 && g_releases == r0 && g_live == 1);
  CHECK(b.get() != nullptr && b.cap() == 10 && b.bytes() == 10 * sizeof(double) && b.grew());
  double* const p = b;                        // the implicit conversion the kernels' arguments use
  CHECK(p == b.get());
  p[9] = 1.0;
  // below and at capacity: pointer and capacity stay, grew() is false again
  CHECK(b.reserve(4) == hipSuccess);
  CHECK(b.get() == p && b.cap() == 10 && !b.grew() && g_allocs == a0 + 1 && g_releases == r0);
  CHECK(b.reserve(10) == hipSuccess);
  CHECK(b.get() == p && b.cap() == 10 && !b.grew() && g_allocs == a0 + 1 && g_releases == r0);
  CHECK(b.reserve(0) == hipSuccess);
  CHECK(b.get() == p && b.cap() == 10 && !b.grew());
  // above capacity: exactly one release, then exactly one allocation
  CHECK(b.reserve(11) == hipSuccess);
  CHECK(g_allocs == a0 + 2 && g_releases == r0 + 1 && g_live == 1);
  CHECK(b.cap() == 11 && b.grew());
  b.get()[10] = 2.0;
  // a refused reserve: the old block is gone, the buffer is empty, the policy's error comes back
  arm(0);
  CHECK(b.reserve(100) == hipErrorOutOfMemory);
  CHECK(b.get() == nullptr && b.cap() == 0 && b.bytes() == 0 && !b.grew());
  CHECK(g_live == 0 && g_releases == r0 + 2 && g_allocs == a0 + 2);
  // ... and nothing claims room below the old capacity either
  arm(0);
  CHECK(b.reserve(5) == hipErrorOutOfMemory);
  CHECK(b.get() == nullptr && b.cap() == 0);
  // a later reserve succeeds
  arm(-1);
  CHECK(b.reserve(5) == hipSuccess);
  CHECK(b.get() != nullptr && b.cap() == 5 && b.grew() && g_live == 1);
  b.get()[4] = 3.0;
  // reset empties; a second reset is harmless
  b.reset();
  CHECK(b.get() == nullptr && b.cap() == 0 && !b.grew() && g_live == 0);
  b.reset();
  CHECK(g_live == 0);
}

static void check_move_and_swap() {
  arm(-1);
  const int r0 = g_releases;
  {
    t_pin<int> a, b;
    CHECK(a.reserve(3) == hipSuccess && b.reserve(7) == hipSuccess);
    int* const pa = a; int* const pb = b;
    a.swap(b);
    CHECK(a.get() == pb && a.cap() == 7 && b.get() == pa && b.cap() == 3 && g_releases == r0 && g_live == 2);
    // move construction: the source is empty, nothing was released
    t_pin<int> m(std::move(a));
    CHECK(m.get() == pb && m.cap() == 7 && a.get() == nullptr && a.cap() == 0 && g_releases == r0 && g_live == 2);
    // move assignment into an empty buffer: no release
    t_pin<int> e;
    e = std::move(m);
    CHECK(e.get() == pb && e.cap() == 7 && m.get() == nullptr && g_releases == r0);
    // move assignment over a block: that block alone goes
    b = std::move(e);
    CHECK(b.get() == pb && b.cap() == 7 && e.get() == nullptr && g_releases == r0 + 1 && g_live == 1);
    b.get()[6] = 1;
    // a local handed over to a member, as host_frames_setup does
    struct holder { t_pin<int> h; } H;
    H.h.swap(b);
    CHECK(H.h.get() == pb && b.get() == nullptr && g_releases == r0 + 1 && g_live == 1);
  }
  CHECK(g_live == 0 && g_releases == r0 + 2);
}

// a workspace like the units': buffers of both policies, a plain pointer into one of them, a zero-fill between allocations
struct test_ws {
  int cap = 0;
  t_dev<float> d_p;
  t_dev<unsigned char> d_mask;
  t_pin<double> h_out;
  t_dev<double> d_out;
  double* d_tail = nullptr;     // into d_out
};

static int32_t build_ws(test_ws& w, int n) {
  w.cap = n;
  if (w.d_p.reserve(4 * (size_t)n) != hipSuccess) return -4;
  if (w.d_mask.reserve((size_t)n) != hipSuccess) return -4;
  memset(w.d_mask, 0, w.d_mask.bytes());
  if (w.h_out.reserve(8) != hipSuccess) return -4;
  if (w.d_out.reserve(8) != hipSuccess) return -4;
  w.d_tail = w.d_out + 4;
  return 0;
}

static void check_ws_replace() {
  const int n_bufs = 4;
  for (int fail = -1; fail < n_bufs; fail++) {
    CHECK(g_live == 0);
    test_ws* slot = nullptr;
    arm(fail);
    const int32_t r = vo_ws_replace(slot, [](test_ws& w) { return build_ws(w, 16); });
    if (fail < 0) {
      // no failure: the slot holds a complete workspace, whose deletion releases every block
      CHECK(r == 0 && slot != nullptr && g_live == n_bufs);
      CHECK(slot->cap == 16 && slot->d_p.cap() == 64 && slot->d_mask.cap() == 16 && slot->h_out.cap() == 8 && slot->d_out.cap() == 8);
      slot->d_tail[3] = 1.0;
      delete slot;
      slot = nullptr;
      CHECK(g_live == 0);
    } else {
      // a failure at any position: the slot stays null and the partial workspace is gone with what it had allocated
      CHECK(r == -4 && slot == nullptr && g_live == 0);
      // the next call starts afresh and succeeds
      arm(-1);
      CHECK(vo_ws_replace(slot, [](test_ws& w) { return build_ws(w, 16); }) == 0);
      CHECK(slot != nullptr && g_live == n_bufs);
      delete slot;
      CHECK(g_live == 0);
    }
  }
  // a build that fails without having allocated
  test_ws* slot = nullptr;
  CHECK(vo_ws_replace(slot, [](test_ws&) { return (int32_t)-2; }) == -2 && slot == nullptr && g_live == 0);
}

// the output rows of a detector: two buffers of one row stride, the stride non-zero only while both hold it
struct pair_ws {
  t_dev<long> d_fin;
  t_dev<float> d_desc;
  int fin_cap = 0;
};
static int32_t pair_reserve(pair_ws& w, int max_out) {
  if (w.fin_cap < max_out) {
    w.fin_cap = 0;
    if (w.d_fin.reserve((size_t)max_out) != hipSuccess) return -4;
    if (w.d_desc.reserve(128 * (size_t)max_out) != hipSuccess) return -4;
    w.fin_cap = max_out;
  }
  return 0;
}
static bool pair_sound(const pair_ws& w) {     // neither the stride nor a capacity claims room that is not there
  return w.d_fin.cap() >= (size_t)w.fin_cap && w.d_desc.cap() >= 128 * (size_t)w.fin_cap &&
         (w.d_fin.cap() == 0) == (w.d_fin.get() == nullptr) && (w.d_desc.cap() == 0) == (w.d_desc.get() == nullptr);
}

static void check_paired() {
  for (int fail = 0; fail < 2; fail++) {
    pair_ws w;
    arm(-1);
    CHECK(pair_reserve(w, 8) == 0 && w.fin_cap == 8 && pair_sound(w) && g_live == 2);
    arm(fail);                               // the first or the second of the two reserves of a regrow is refused
    CHECK(pair_reserve(w, 32) == -4);
    CHECK(w.fin_cap == 0 && pair_sound(w));
    if (fail == 1) CHECK(w.d_fin.cap() == 32 && w.d_desc.cap() == 0 && w.d_desc.get() == nullptr && g_live == 1);
    // a later call with a SMALLER max_out does not take the rows for built: it reserves again, and both hold the stride
    arm(-1);
    CHECK(pair_reserve(w, 4) == 0 && w.fin_cap == 4 && pair_sound(w));
    w.d_desc.get()[128 * 4 - 1] = 1.f;
    w.d_fin.get()[3] = 1;
    CHECK(pair_reserve(w, 32) == 0 && w.fin_cap == 32 && pair_sound(w) && g_live == 2);
    w.d_desc.get()[128 * 32 - 1] = 1.f;
  }
  CHECK(g_live == 0);
}

int main() {
  check_reserve();
  check_move_and_swap();
  check_ws_replace();
  check_paired();
  CHECK(g_live == 0 && g_allocs == g_releases);
  printf("vo_buf_check OK: %d allocations, %d releases\n", g_allocs, g_releases);
  return 0;
}
