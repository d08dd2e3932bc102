// driver.cpp — a compiled caller of the C ABI's asynchronous batches: the loop a cgo host runs
// (submit, keep `depth` batches in flight, wait for the oldest), so that bench.py can time the
// engine through C calls instead of one ctypes round trip per call (~3-4 us each in CPython,
// ~0.1 us through cgo). It calls only gck_check_submit / gck_check_wait, through the pointers the
// caller passes (the entry points of the libgck instance that created the engine), so it never
// links a second copy of the library.
//   built by make -C gochugaru_amd/csrc as gochugaru_amd/libgck_driver.so
#include <chrono>
#include <cstdint>
#include <deque>

#include "gck.h"

using submit_fn = int (*)(gck_engine*, const gck_consistency*, const gck_item*, size_t, const char* const*,
                          const size_t*, size_t, int64_t, uint8_t*, int32_t*, uint32_t, void*, gck_batch**);
using wait_fn = int (*)(gck_engine*, gck_batch*);
using submit_uniform_fn = int (*)(gck_engine*, const gck_consistency*, const gck_uniform*, const uint32_t*, size_t,
                                  const char* const*, const size_t*, size_t, int64_t, uint64_t*, gck_item_error*,
                                  size_t, size_t*, gck_batch**);
using submit_shaped_fn = int (*)(gck_engine*, const gck_consistency*, const gck_uniform*, size_t, const uint8_t*,
                                 const uint32_t*, size_t, const char* const*, const size_t*, size_t, int64_t, uint64_t*,
                                 gck_item_error*, size_t, size_t*, gck_batch**);
using submit_cross_fn = int (*)(gck_engine*, const gck_consistency*, const gck_uniform*, const uint32_t*, size_t,
                                const uint32_t*, size_t, const char* const*, const size_t*, size_t, int64_t, uint64_t*,
                                gck_item_error*, size_t, size_t*, gck_batch**);
using submit_list_fn = int (*)(gck_engine*, const gck_consistency*, const gck_uniform*, uint32_t, uint32_t,
                               const uint32_t*, uint32_t, size_t, const char* const*, const size_t*, size_t, int64_t,
                               uint64_t*, gck_item_error*, size_t, size_t*, gck_batch**);
using submit_uniform_device_fn = int (*)(gck_engine*, const gck_consistency*, const gck_uniform*, const uint32_t*, size_t,
                                         const char* const*, const size_t*, size_t, int64_t, uint64_t*, gck_item_error*,
                                         size_t, uint32_t*, uint32_t, void*, gck_batch**);
using submit_list_device_fn = int (*)(gck_engine*, const gck_consistency*, const gck_uniform*, uint32_t, uint32_t,
                                      const uint32_t*, uint32_t, size_t, const char* const*, const size_t*, size_t,
                                      int64_t, uint64_t*, gck_item_error*, size_t, uint32_t*, uint32_t, void*,
                                      gck_batch**);
using submit_cross_device_fn = int (*)(gck_engine*, const gck_consistency*, const gck_uniform*, const uint32_t*, size_t,
                                       const uint32_t*, size_t, const char* const*, const size_t*, size_t, int64_t,
                                       uint64_t*, gck_item_error*, size_t, uint32_t*, uint32_t, void*, gck_batch**);
using submit_filter_device_fn = int (*)(gck_engine*, const gck_consistency*, const gck_uniform*, uint32_t, uint32_t,
                                        const uint32_t*, uint32_t, size_t, const char* const*, const size_t*, size_t,
                                        int64_t, const gck_select*, uint64_t*, gck_item_error*, size_t, uint32_t*,
                                        uint32_t, void*, gck_batch**);
using submit_filter_cross_device_fn = int (*)(gck_engine*, const gck_consistency*, const gck_uniform*, const uint32_t*,
                                              size_t, const uint32_t*, size_t, const char* const*, const size_t*, size_t,
                                              int64_t, const gck_select_rows*, uint64_t*, gck_item_error*, size_t,
                                              uint32_t*, uint32_t, void*, gck_batch**);
using submit_filter_cross_cols_device_fn = int (*)(gck_engine*, const gck_consistency*, const gck_uniform*,
                                                   const uint32_t*, size_t, const uint32_t*, size_t, const char* const*,
                                                   const size_t*, size_t, int64_t, const gck_select_cols*, uint64_t*,
                                                   gck_item_error*, size_t, uint32_t*, uint32_t, void*, gck_batch**);

// Optional per-batch timeline of the next loops (gckd_set_trace): for batch k, the seconds after
// the loop's start at which its submit and its wait returned (stamps[2k], stamps[2k + 1]).
static double* g_stamps = nullptr;
static size_t g_cap = 0;

static inline void stamp(std::chrono::steady_clock::time_point t0, size_t k, int which) {
  if (k < g_cap) g_stamps[2 * k + which] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// The loop of every export below: batches k = 0 .. n_batches-1 with up to `depth` in flight (0
// counts as 1); submit_k(k, &b) starts batch k. After an error no further batch is submitted, and
// every submitted batch is still waited for. Returns GCK_OK or the first error; *seconds = wall
// time from the first submit to the last wait.
template <class SubmitK>
static int run_loop(size_t n_batches, uint32_t depth, wait_fn wait, gck_engine* e, double* seconds, SubmitK submit_k) {
  if (depth == 0) depth = 1;
  std::deque<gck_batch*> q;
  int rc = GCK_OK;
  size_t kw = 0;  // batches waited for so far: the oldest in flight is batch kw
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t k = 0; k < n_batches && rc == GCK_OK; ++k) {
    if (q.size() >= depth) {
      rc = wait(e, q.front());
      stamp(t0, kw++, 1);
      q.pop_front();
      if (rc != GCK_OK) break;
    }
    gck_batch* b = nullptr;
    rc = submit_k(k, &b);
    if (rc == GCK_OK) q.push_back(b);
    stamp(t0, k, 0);
  }
  while (!q.empty()) {  // every submitted batch is waited for, also after an error
    const int r = wait(e, q.front());
    stamp(t0, kw++, 1);
    if (rc == GCK_OK) rc = r;
    q.pop_front();
  }
  if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

extern "C" {

void gckd_set_trace(double* stamps, size_t n_batches) {
  g_stamps = stamps;
  g_cap = stamps ? n_batches : 0;
}

// Batches over device buffers items[k], perm[k], err[k], n checks each; batch k is submitted on
// streams[k % depth] with GCK_SUBMIT_DEVICE | flags (GCK_SUBMIT_ENGINE_STREAM: on the engine's
// workspace streams instead), at now_us (0 = the clock).
int gckd_run(submit_fn submit, wait_fn wait, gck_engine* e, const gck_consistency* cs, size_t n_batches, const uint64_t* items,
             const uint64_t* perm, const uint64_t* err, size_t n, uint32_t depth, const uint64_t* streams,
             uint32_t flags, int64_t now_us, double* seconds) {
  if (depth == 0) depth = 1;
  return run_loop(n_batches, depth, wait, e, seconds, [&](size_t k, gck_batch** b) {
    return submit(e, cs, reinterpret_cast<const gck_item*>(items[k]), n, nullptr, nullptr, 0, now_us,
                  reinterpret_cast<uint8_t*>(perm[k]), reinterpret_cast<int32_t*>(err[k]), GCK_SUBMIT_DEVICE | flags,
                  reinterpret_cast<void*>(streams[k % depth]), b);
  });
}

// The same loop over host buffers (no GCK_SUBMIT_DEVICE): items[k] / perm[k] / err[k] are host
// pointers — gck_host_alloc memory moves by DMA straight from and into them — and each batch runs
// on the engine's workspace stream: items H2D, kernels, results D2H.
int gckd_run_host(submit_fn submit, wait_fn wait, gck_engine* e, const gck_consistency* cs, size_t n_batches,
                  const uint64_t* items, const uint64_t* perm, const uint64_t* err, size_t n, uint32_t depth,
                  int64_t now_us, double* seconds) {
  return run_loop(n_batches, depth, wait, e, seconds, [&](size_t k, gck_batch** b) {
    return submit(e, cs, reinterpret_cast<const gck_item*>(items[k]), n, nullptr, nullptr, 0, now_us,
                  reinterpret_cast<uint8_t*>(perm[k]), reinterpret_cast<int32_t*>(err[k]), 0u, nullptr, b);
  });
}

// The same loop over uniform requests (gck_check_submit_uniform): request k = header hdrs[k] and
// ns[k] host pairs pairs[k] (u32 ids) in, packed[k] (ceil(ns[k] / 32) words) and errs[k] (err_cap
// records, the count in n_errs[k]) out — what Client.Check sends for runs of relationships of one
// shape, 8 B per check.
int gckd_run_uniform(submit_uniform_fn submit, wait_fn wait, gck_engine* e, const gck_consistency* cs, size_t n_batches,
                     const gck_uniform* hdrs, const uint64_t* pairs, const uint64_t* ns, const uint64_t* packed,
                     const uint64_t* errs, size_t err_cap, size_t* n_errs, uint32_t depth, int64_t now_us,
                     double* seconds) {
  return run_loop(n_batches, depth, wait, e, seconds, [&](size_t k, gck_batch** b) {
    return submit(e, cs, hdrs + k, reinterpret_cast<const uint32_t*>(pairs[k]), (size_t)ns[k], nullptr, nullptr, 0,
                  now_us, reinterpret_cast<uint64_t*>(packed[k]), reinterpret_cast<gck_item_error*>(errs[k]), err_cap,
                  n_errs ? n_errs + k : nullptr, b);
  });
}

// The same loop over shaped requests (gck_check_submit_shaped): request k = the table shapes[k]
// (n_shapes[k] gck_uniform entries), the index bytes shape_of[k] and ns[k] host pairs pairs[k] in;
// the outputs as gckd_run_uniform's — what Client.Check sends for relationships of mixed shapes,
// 9 B per check.
int gckd_run_shaped(submit_shaped_fn submit, wait_fn wait, gck_engine* e, const gck_consistency* cs, size_t n_batches,
                    const uint64_t* shapes, const uint64_t* n_shapes, const uint64_t* shape_of, const uint64_t* pairs,
                    const uint64_t* ns, const uint64_t* packed, const uint64_t* errs, size_t err_cap, size_t* n_errs,
                    uint32_t depth, int64_t now_us, double* seconds) {
  return run_loop(n_batches, depth, wait, e, seconds, [&](size_t k, gck_batch** b) {
    return submit(e, cs, reinterpret_cast<const gck_uniform*>(shapes[k]), (size_t)n_shapes[k],
                  reinterpret_cast<const uint8_t*>(shape_of[k]), reinterpret_cast<const uint32_t*>(pairs[k]), (size_t)ns[k],
                  nullptr, nullptr, 0, now_us, reinterpret_cast<uint64_t*>(packed[k]),
                  reinterpret_cast<gck_item_error*>(errs[k]), err_cap, n_errs ? n_errs + k : nullptr, b);
  });
}

// The same loop over cross requests (gck_check_submit_cross): request k = header hdrs[k], the
// n_subjects[k] subject ids subjects[k] and the n_resources[k] resource ids resources[k] in;
// packed[k] (n_subjects[k] rows of ceil(n_resources[k] / 32) words) and errs[k] out — 4 B per id
// instead of 8 B per check.
int gckd_run_cross(submit_cross_fn submit, wait_fn wait, gck_engine* e, const gck_consistency* cs, size_t n_batches,
                   const gck_uniform* hdrs, const uint64_t* subjects, const uint64_t* n_subjects,
                   const uint64_t* resources, const uint64_t* n_resources, const uint64_t* packed, const uint64_t* errs,
                   size_t err_cap, size_t* n_errs, uint32_t depth, int64_t now_us, double* seconds) {
  return run_loop(n_batches, depth, wait, e, seconds, [&](size_t k, gck_batch** b) {
    return submit(e, cs, hdrs + k, reinterpret_cast<const uint32_t*>(subjects[k]), (size_t)n_subjects[k],
                  reinterpret_cast<const uint32_t*>(resources[k]), (size_t)n_resources[k], nullptr, nullptr, 0, now_us,
                  reinterpret_cast<uint64_t*>(packed[k]), reinterpret_cast<gck_item_error*>(errs[k]), err_cap,
                  n_errs ? n_errs + k : nullptr, b);
  });
}

// The same loop over list requests (gck_check_submit_list): request k = header hdrs[k], the fixed
// id fixed[k] on the side `vary` leaves, and ns[k] varying ids — the host list ids[k], or with
// ids[k] == 0 the range from first[k] — in; packed[k] (ceil(ns[k] / 32) words) and errs[k] out: 4 or
// 0 B per check instead of 8.
int gckd_run_list(submit_list_fn submit, wait_fn wait, gck_engine* e, const gck_consistency* cs, size_t n_batches,
                  const gck_uniform* hdrs, const uint32_t* fixed, uint32_t vary, const uint64_t* ids,
                  const uint32_t* first, const uint64_t* ns, const uint64_t* packed, const uint64_t* errs,
                  size_t err_cap, size_t* n_errs, uint32_t depth, int64_t now_us, double* seconds) {
  return run_loop(n_batches, depth, wait, e, seconds, [&](size_t k, gck_batch** b) {
    return submit(e, cs, hdrs + k, fixed[k], vary, reinterpret_cast<const uint32_t*>(ids[k]), first[k], (size_t)ns[k],
                  nullptr, nullptr, 0, now_us, reinterpret_cast<uint64_t*>(packed[k]),
                  reinterpret_cast<gck_item_error*>(errs[k]), err_cap, n_errs ? n_errs + k : nullptr, b);
  });
}

// The uniform loop over device buffers (gck_check_submit_uniform_device): pairs[k], packed[k],
// errs[k] and n_errs[k] (0: no count word) are device pointers; request k is submitted on
// streams[k % depth], or with flags = GCK_SUBMIT_ENGINE_STREAM on the engine's workspace streams.
int gckd_run_uniform_device(submit_uniform_device_fn submit, wait_fn wait, gck_engine* e, const gck_consistency* cs,
                            size_t n_batches, const gck_uniform* hdrs, const uint64_t* pairs, const uint64_t* ns,
                            const uint64_t* packed, const uint64_t* errs, size_t err_cap, const uint64_t* n_errs,
                            uint32_t depth, const uint64_t* streams, uint32_t flags, int64_t now_us, double* seconds) {
  if (depth == 0) depth = 1;
  return run_loop(n_batches, depth, wait, e, seconds, [&](size_t k, gck_batch** b) {
    return submit(e, cs, hdrs + k, reinterpret_cast<const uint32_t*>(pairs[k]), (size_t)ns[k], nullptr, nullptr, 0,
                  now_us, reinterpret_cast<uint64_t*>(packed[k]), reinterpret_cast<gck_item_error*>(errs[k]), err_cap,
                  reinterpret_cast<uint32_t*>(n_errs[k]), flags, reinterpret_cast<void*>(streams[k % depth]), b);
  });
}

// ... and the list loop (gck_check_submit_list_device): ids[k] is a device id list, or 0 for the
// range from first[k].
int gckd_run_list_device(submit_list_device_fn submit, wait_fn wait, gck_engine* e, const gck_consistency* cs,
                         size_t n_batches, const gck_uniform* hdrs, const uint32_t* fixed, uint32_t vary,
                         const uint64_t* ids, const uint32_t* first, const uint64_t* ns, const uint64_t* packed,
                         const uint64_t* errs, size_t err_cap, const uint64_t* n_errs, uint32_t depth,
                         const uint64_t* streams, uint32_t flags, int64_t now_us, double* seconds) {
  if (depth == 0) depth = 1;
  return run_loop(n_batches, depth, wait, e, seconds, [&](size_t k, gck_batch** b) {
    return submit(e, cs, hdrs + k, fixed[k], vary, reinterpret_cast<const uint32_t*>(ids[k]), first[k], (size_t)ns[k],
                  nullptr, nullptr, 0, now_us, reinterpret_cast<uint64_t*>(packed[k]),
                  reinterpret_cast<gck_item_error*>(errs[k]), err_cap, reinterpret_cast<uint32_t*>(n_errs[k]), flags,
                  reinterpret_cast<void*>(streams[k % depth]), b);
  });
}

// ... and the cross loop (gck_check_submit_cross_device): subjects[k] and resources[k] are device id
// lists (one buffer in block layout, or two), packed[k] the row-padded plane in device memory.
int gckd_run_cross_device(submit_cross_device_fn submit, wait_fn wait, gck_engine* e, const gck_consistency* cs,
                          size_t n_batches, const gck_uniform* hdrs, const uint64_t* subjects, const uint64_t* n_subjects,
                          const uint64_t* resources, const uint64_t* n_resources, const uint64_t* packed,
                          const uint64_t* errs, size_t err_cap, const uint64_t* n_errs, uint32_t depth,
                          const uint64_t* streams, uint32_t flags, int64_t now_us, double* seconds) {
  if (depth == 0) depth = 1;
  return run_loop(n_batches, depth, wait, e, seconds, [&](size_t k, gck_batch** b) {
    return submit(e, cs, hdrs + k, reinterpret_cast<const uint32_t*>(subjects[k]), (size_t)n_subjects[k],
                  reinterpret_cast<const uint32_t*>(resources[k]), (size_t)n_resources[k], nullptr, nullptr, 0, now_us,
                  reinterpret_cast<uint64_t*>(packed[k]), reinterpret_cast<gck_item_error*>(errs[k]), err_cap,
                  reinterpret_cast<uint32_t*>(n_errs[k]), flags, reinterpret_cast<void*>(streams[k % depth]), b);
  });
}

// The list loop with the survivors compacted on the device (gck_filter_submit_list_device): request k
// also has its own outputs — out_ids[k], out_pos[k], out_perm[k] (cap entries each; 0: not wanted)
// and the count word out_n[k] — under the one mask; packed[k] may be 0.
int gckd_run_filter_device(submit_filter_device_fn submit, wait_fn wait, gck_engine* e, const gck_consistency* cs,
                           size_t n_batches, const gck_uniform* hdrs, const uint32_t* fixed, uint32_t vary,
                           const uint64_t* ids, const uint32_t* first, const uint64_t* ns, uint32_t mask,
                           const uint64_t* out_ids, const uint64_t* out_pos, const uint64_t* out_perm, size_t cap,
                           const uint64_t* out_n, const uint64_t* packed, const uint64_t* errs, size_t err_cap,
                           const uint64_t* n_errs, uint32_t depth, const uint64_t* streams, uint32_t flags,
                           int64_t now_us, double* seconds) {
  if (depth == 0) depth = 1;
  return run_loop(n_batches, depth, wait, e, seconds, [&](size_t k, gck_batch** b) {
    gck_select sel{};  // (copied by the call)
    sel.mask = mask;
    sel.d_out_ids = reinterpret_cast<uint32_t*>(out_ids[k]);
    sel.d_out_pos = reinterpret_cast<uint32_t*>(out_pos[k]);
    sel.d_out_perm = reinterpret_cast<uint8_t*>(out_perm[k]);
    sel.cap = cap;
    sel.d_out_n = reinterpret_cast<uint32_t*>(out_n[k]);
    return submit(e, cs, hdrs + k, fixed[k], vary, reinterpret_cast<const uint32_t*>(ids[k]), first[k], (size_t)ns[k],
                  nullptr, nullptr, 0, now_us, &sel, reinterpret_cast<uint64_t*>(packed[k]),
                  reinterpret_cast<gck_item_error*>(errs[k]), err_cap, reinterpret_cast<uint32_t*>(n_errs[k]), flags,
                  reinterpret_cast<void*>(streams[k % depth]), b);
  });
}

// The cross loop with each subject's survivors compacted on the device (gck_filter_submit_cross_device):
// request k also has its own CSR — row_off[k] (n_subjects[k] + 1 entries), row_n[k], out_ids[k],
// out_col[k], out_perm[k] (cap entries each; 0: not wanted) and the count word out_n[k] — under the
// one mask and row limit.
int gckd_run_filter_cross_device(submit_filter_cross_device_fn submit, wait_fn wait, gck_engine* e,
                                 const gck_consistency* cs, size_t n_batches, const gck_uniform* hdrs,
                                 const uint64_t* subjects, const uint64_t* n_subjects, const uint64_t* resources,
                                 const uint64_t* n_resources, uint32_t mask, uint32_t row_limit, const uint64_t* row_off,
                                 const uint64_t* row_n, const uint64_t* out_ids, const uint64_t* out_col,
                                 const uint64_t* out_perm, size_t cap, const uint64_t* out_n, const uint64_t* packed,
                                 const uint64_t* errs, size_t err_cap, const uint64_t* n_errs, uint32_t depth,
                                 const uint64_t* streams, uint32_t flags, int64_t now_us, double* seconds) {
  if (depth == 0) depth = 1;
  return run_loop(n_batches, depth, wait, e, seconds, [&](size_t k, gck_batch** b) {
    gck_select_rows sel{};  // (copied by the call)
    sel.mask = mask;
    sel.row_limit = row_limit;
    sel.d_out_row_off = reinterpret_cast<uint32_t*>(row_off[k]);
    sel.d_out_row_n = reinterpret_cast<uint32_t*>(row_n[k]);
    sel.d_out_ids = reinterpret_cast<uint32_t*>(out_ids[k]);
    sel.d_out_col = reinterpret_cast<uint32_t*>(out_col[k]);
    sel.d_out_perm = reinterpret_cast<uint8_t*>(out_perm[k]);
    sel.cap = cap;
    sel.d_out_n = reinterpret_cast<uint32_t*>(out_n[k]);
    return submit(e, cs, hdrs + k, reinterpret_cast<const uint32_t*>(subjects[k]), (size_t)n_subjects[k],
                  reinterpret_cast<const uint32_t*>(resources[k]), (size_t)n_resources[k], nullptr, nullptr, 0, now_us,
                  &sel, reinterpret_cast<uint64_t*>(packed[k]), reinterpret_cast<gck_item_error*>(errs[k]), err_cap,
                  reinterpret_cast<uint32_t*>(n_errs[k]), flags, reinterpret_cast<void*>(streams[k % depth]), b);
  });
}

// Its twin by resource (gck_filter_submit_cross_cols_device): request k's CSR is col_off[k]
// (n_resources[k] + 1 entries), col_n[k], out_ids[k], out_row[k], out_perm[k] (cap entries each; 0: not
// wanted) and the count word out_n[k], under the one mask and column limit.
int gckd_run_filter_cross_cols_device(submit_filter_cross_cols_device_fn submit, wait_fn wait, gck_engine* e,
                                      const gck_consistency* cs, size_t n_batches, const gck_uniform* hdrs,
                                      const uint64_t* subjects, const uint64_t* n_subjects, const uint64_t* resources,
                                      const uint64_t* n_resources, uint32_t mask, uint32_t col_limit,
                                      const uint64_t* col_off, const uint64_t* col_n, const uint64_t* out_ids,
                                      const uint64_t* out_row, const uint64_t* out_perm, size_t cap, const uint64_t* out_n,
                                      const uint64_t* packed, const uint64_t* errs, size_t err_cap, const uint64_t* n_errs,
                                      uint32_t depth, const uint64_t* streams, uint32_t flags, int64_t now_us,
                                      double* seconds) {
  if (depth == 0) depth = 1;
  return run_loop(n_batches, depth, wait, e, seconds, [&](size_t k, gck_batch** b) {
    gck_select_cols sel{};  // (copied by the call)
    sel.mask = mask;
    sel.col_limit = col_limit;
    sel.d_out_col_off = reinterpret_cast<uint32_t*>(col_off[k]);
    sel.d_out_col_n = reinterpret_cast<uint32_t*>(col_n[k]);
    sel.d_out_ids = reinterpret_cast<uint32_t*>(out_ids[k]);
    sel.d_out_row = reinterpret_cast<uint32_t*>(out_row[k]);
    sel.d_out_perm = reinterpret_cast<uint8_t*>(out_perm[k]);
    sel.cap = cap;
    sel.d_out_n = reinterpret_cast<uint32_t*>(out_n[k]);
    return submit(e, cs, hdrs + k, reinterpret_cast<const uint32_t*>(subjects[k]), (size_t)n_subjects[k],
                  reinterpret_cast<const uint32_t*>(resources[k]), (size_t)n_resources[k], nullptr, nullptr, 0, now_us,
                  &sel, reinterpret_cast<uint64_t*>(packed[k]), reinterpret_cast<gck_item_error*>(errs[k]), err_cap,
                  reinterpret_cast<uint32_t*>(n_errs[k]), flags, reinterpret_cast<void*>(streams[k % depth]), b);
  });
}

}  // extern "C"
