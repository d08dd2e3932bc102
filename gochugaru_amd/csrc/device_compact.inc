// Compact requests over device buffers (include/gck.h gck_check_bulk_uniform_device ...): what the
// host does for a compact request over host buffers — expanding a chunk to items, packing the
// 2-bit words, patching the checks the join left into them, listing the errors in ascending order
// (compact_expand, uniform_collect, uniform_errors) — done by kernels, so that no per-check data
// crosses PCIe. Included by engine.hip.
//
// In place (CompactRun::kInPlace with `device`): the join reads the caller's pairs / index bytes /
// id list and writes the caller's plane; the checks it leaves are answered by the bundle stages
// into the workspace's d_perm / d_err, and k_dc_patch + k_dc_emit put them into the plane and the
// error list — only when the join left checks, so the common batch has no launch beyond its join.
// Expanded (kExpanded with `device`): k_dc_expand writes the chunk's items into the workspace's item
// array, the chunk runs as a device batch into d_perm / d_err, and k_dc_pack + k_dc_emit write the
// plane and the list.
//
// The error list: a per-workspace bitmap, one bit per check of the chunk (set by k_dc_patch or
// k_dc_pack, cleared by k_dc_emit, so it is zero between batches), turned into records by one block:
// popcount per word, an exclusive scan over the block, records at base + rank while below err_cap.
// `base` is the request's count so far on the device (the caller's *d_out_n_errs, or the word of the
// request's first workspace), so the chunks of a request, emitted in chunk order, accumulate.
//
// A filter request (gck_filter_list_device) adds k_dc_select behind them, for every batch: the
// survivors of the finished plane, in the caller's order, at their ranks in the request.
//
// A cross request (gck_check_bulk_cross_device) in place is cut into full-width tiles — `rows`
// subjects by all R resources — so a tile's dense words are the run of the caller's plane that begins
// at its first row, and its padded check order is the request's s * R + r order: the join writes the
// caller's plane, after k_dc_cross_ids has put the tile's ids into the workspace's id block (or reads
// the caller's own buffer when that is in block layout already), and k_dc_emit maps a padded index to
// the request's. Expanded, its chunks of the row-major sequence end inside plane words, so the plane
// is cleared once and k_dc_cross_pack ORs each result into its word.
//
// A group filter request (gck_filter_groups_device) is a uniform device request whose pairs a kernel
// writes: k_dc_group_pairs expands each chunk's (owner, candidate) pairs from the caller's CSR into the
// workspace's dc_pairs, the chunk runs as above, and the group-segmented selection follows the last one.

// The shapes of a request, by value in the kernarg segment (a uniform or list request: one entry).
struct DcShapes {
  gck_uniform s[GCK_MAX_SHAPES];
};

struct DcExpand {
  const uint32_t* ids;      // the chunk's pairs (8 B per check), or a list chunk's ids (4 B), or null: a range
  const uint8_t* shape_of;  // the chunk's index bytes; null: every check is shape 0
  gck_item* items;          // out: n items
  uint32_t* bad;            // the smallest check of the chunk whose index byte is beyond the table (atomic min)
  uint32_t n, n_shapes;
  uint32_t vary;            // 0: pairs; GCK_VARY_RESOURCE / GCK_VARY_SUBJECT: a list chunk
  uint32_t fixed_id, first_id;
  // a cross request's chunk (R != 0): `ids` is the whole resource list, `subs` the whole subject list,
  // and check i of the chunk is check pos + i of the request (pos + n <= S * R < 2^32)
  const uint32_t* subs;
  uint32_t R, pos;
};

// compact_expand on the device: check i of the chunk as a 20-B item. A check whose index byte is
// beyond the table becomes shape 0's item (harmless: the request fails afterwards).
__global__ void k_dc_expand(DcExpand a, DcShapes t) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  uint32_t s = a.shape_of ? a.shape_of[i] : 0u;
  if (s >= a.n_shapes) {
    atomicMin(a.bad, i);
    s = 0u;
  }
  const gck_uniform h = t.s[s];
  uint32_t res, sub;
  if (a.R) {
    const uint32_t g = a.pos + i;
    res = a.ids[g % a.R];
    sub = a.subs[g / a.R];
  } else if (a.vary) {
    const uint32_t v = a.ids ? a.ids[i] : a.first_id + i;
    res = a.vary == GCK_VARY_SUBJECT ? a.fixed_id : v;
    sub = a.vary == GCK_VARY_SUBJECT ? v : a.fixed_id;
  } else {
    res = a.ids[2ull * i];
    sub = a.ids[2ull * i + 1];
  }
  gck_item it;
  it.resource_type = h.resource_type;
  it.permission = h.permission;
  it.resource_id = res;
  it.subject_type = h.subject_type;
  it.subject_relation = h.subject_relation;
  it.subject_id = sub;
  it.context_slot = h.context_slot;
  a.items[i] = it;
}

// The chunk's results as 2-bit words and its error bits: a wave takes 64 checks, that is two words,
// each half-wave OR-reducing its 32 results; lanes 0 and 32 write. Every word of the chunk
// (ceil(n / 32)) is written, tail bits 0 (lanes beyond n contribute nothing).
__global__ void k_dc_pack(const uint8_t* perm, const int32_t* err, uint32_t n, unsigned long long* out, uint32_t* bitmap) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t l = threadIdx.x & 31u;
  const bool in = i < n;
  const bool bad = in && err[i] != 0;
  const uint32_t v = in && !bad ? (uint32_t)perm[i] & 3u : 0u;
  uint32_t lo = l < 16u ? v << (2u * l) : 0u, hi = l >= 16u ? v << (2u * (l - 16u)) : 0u;
  for (int d = 16; d >= 1; d >>= 1) {
    lo |= (uint32_t)__shfl_xor((int)lo, d, 32);
    hi |= (uint32_t)__shfl_xor((int)hi, d, 32);
  }
  const unsigned long long bits = __ballot(bad);
  const uint32_t word = i >> 5, words = (n + 31u) / 32u;  // (n <= max_batch: no overflow)
  if (l == 0u && word < words) {
    out[word] = (unsigned long long)hi << 32 | lo;
    bitmap[word] = (threadIdx.x & 32u) ? (uint32_t)(bits >> 32) : (uint32_t)bits;
  }
}

// A cross tile's ids into the workspace's id block, in the layout its join reads (closure.inc
// cross_ids): the R resource ids at word 0, the tile's `rows` subject ids from word cross_sub_off(R).
// One thread per id; the host has checked cross_sub_off(R) + rows against the block. `zero`: the
// request's count word, cleared here when the batch's emit follows this kernel on its stream (null:
// cleared elsewhere).
__global__ void k_dc_cross_ids(const uint32_t* resources, uint32_t R, const uint32_t* subjects, uint32_t rows,
                               uint32_t* block, uint32_t* zero) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0 && zero) *zero = 0u;
  if (t < R) block[t] = resources[t];
  else if (t - R < rows) block[cross_sub_off(R) + (t - R)] = subjects[t - R];
}

// An expanded cross chunk's results into the row-padded plane, and its error bits: check i of the
// chunk is check g = pos + i of the request, subject g / R against resource g % R. The plane was
// cleared before the request's first chunk, and a word may be shared by two chunks (a chunk ends
// inside a row), so each non-zero result is OR-ed into its word. The bitmap is k_dc_pack's: one bit
// per check of the chunk, a ballot per half-wave, every one of its ceil(n / 32) words written.
__global__ void k_dc_cross_pack(const uint8_t* perm, const int32_t* err, uint32_t n, uint32_t pos, uint32_t R,
                                uint32_t stride, unsigned long long* plane, uint32_t* bitmap) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n;
  const bool bad = in && err[i] != 0;
  const uint32_t v = in && !bad ? (uint32_t)perm[i] & 3u : 0u;
  if (v) {
    const uint32_t g = pos + i, s = g / R, r = g - s * R;  // (g < S * R: s < S, and r / 32 < stride)
    atomicOr(&plane[(size_t)s * stride + (r >> 5)], (unsigned long long)v << (2u * (r & 31u)));
  }
  const unsigned long long bits = __ballot(bad);
  const uint32_t word = i >> 5, words = (n + 31u) / 32u;
  if ((threadIdx.x & 31u) == 0u && word < words)
    bitmap[word] = (threadIdx.x & 32u) ? (uint32_t)(bits >> 32) : (uint32_t)bits;
}

// The checks the join of an in-place chunk left (its deferred list, n_left entries), answered by the
// bundle stages into perm / err: an error sets the check's bit of the bitmap, a result is OR-ed
// into the plane — the join wrote 0 there, and two such checks may share a word.
__global__ void k_dc_patch(const uint32_t* left, uint32_t n_left, uint32_t n, const uint8_t* perm, const int32_t* err,
                           unsigned long long* out, uint32_t* bitmap) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_left) return;
  const uint32_t i = left[k];
  if (i >= n) return;
  if (err[i] != 0) {
    atomicOr(&bitmap[i >> 5], 1u << (i & 31u));
  } else {
    const unsigned long long v = (unsigned long long)(perm[i] & 3u) << (2u * (i & 31u));
    if (v) atomicOr(&out[i >> 5], v);
  }
}

// The bitmap's `words` words as ascending (index, code) records: one block, a tile of blockDim words
// at a time. Record r of the request (r counts from *count, the chunks before this one) is written
// while r < cap; *count becomes the request's count so far. Clears the bitmap.
// The index of check i of the chunk in its request is pos + i — or, for a cross tile read in place
// (row_len != 0: the padded checks of a tile row, 32 * ceil(R / 32); pos = row0 * R), pos +
// (i / row_len) * R + i % row_len: below S * R < 2^32, since a padding lane sets no bit.
__global__ void k_dc_emit(uint32_t* bitmap, uint32_t words, const int32_t* err, uint32_t pos, gck_item_error* out,
                          uint32_t cap, uint32_t* count, uint32_t row_len = 0u, uint32_t R = 0u) {
  __shared__ uint32_t wave_tot[kWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t base = *count;
  __syncthreads();  // (every thread has read the count before thread 0 writes it)
  uint32_t run = 0;
  for (uint32_t t0 = 0; t0 < words; t0 += blockDim.x) {
    const uint32_t t = t0 + threadIdx.x;
    uint32_t word = 0;
    if (t < words) {
      word = bitmap[t];
      if (word) bitmap[t] = 0u;
    }
    const uint32_t pc = __popc(word);
    uint32_t incl = pc;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
      if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63u) wave_tot[wave] = incl;
    __syncthreads();
    uint32_t before = 0, tot = 0;
    for (uint32_t k = 0; k < (uint32_t)kWaves; ++k) {
      if (k < wave) before += wave_tot[k];
      tot += wave_tot[k];
    }
    uint32_t rank = base + run + before + incl - pc;
    while (word) {
      const uint32_t b = (uint32_t)__ffs((int)word) - 1u;
      word &= word - 1u;
      const uint32_t i = t * 32u + b;
      const uint32_t at = row_len ? (i / row_len) * R + i % row_len : i;
      if (rank < cap) out[rank] = gck_item_error{pos + at, err[i]};
      ++rank;
    }
    run += tot;
    __syncthreads();  // (wave_tot is rewritten by the next tile)
  }
  if (threadIdx.x == 0) *count = base + run;
}

// A filter request's chunk (include/gck.h gck_filter_list_device): the survivors of the finished
// plane — the checks whose 2-bit value `mask` selects — as ascending records at their ranks in the
// request (select_plane.hpp). One thread per word, a tile of blockDim words per block. A block's
// first rank is the request's count before this chunk (*prev; null: 0, the first chunk) plus the
// survivors of the words before its tile, which the block counts again itself, plus the exclusive
// scan inside the tile (k_dc_emit's). No block waits on another, and none reads a word another one
// writes: the block of the last tile writes the count so far to *next — never the word `prev`
// names — and to *out_n.
struct DcSelect {
  const unsigned long long* plane;
  uint32_t words, mask;
  gck::SelectOut o;
  const uint32_t* prev;
  uint32_t* next;
  uint32_t* out_n;
};

static_assert(gck::kSelBlock == (uint32_t)kBlock, "the host hook tiles as the kernel's blocks do");

__global__ void __launch_bounds__(kBlock) k_dc_select(DcSelect a) {
  __shared__ uint32_t before_tot[kWaves];
  __shared__ uint32_t wave_tot[kWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t tile0 = blockIdx.x * blockDim.x, t = tile0 + threadIdx.x;
  const uint64_t* plane = reinterpret_cast<const uint64_t*>(a.plane);
  uint32_t mine = gck::select_count_strided(plane, threadIdx.x, tile0, blockDim.x, a.mask);
  for (int d = 32; d >= 1; d >>= 1) mine += (uint32_t)__shfl_xor((int)mine, d, 64);
  const uint64_t word = t < a.words ? plane[t] : 0ull;
  const uint64_t m = gck::select_mask(word, a.mask);
  const uint32_t pc = gck::select_count(m);
  uint32_t incl = pc;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
    if (lane >= (uint32_t)d) incl += up;
  }
  if (lane == 63u) {
    wave_tot[wave] = incl;
    before_tot[wave] = mine;
  }
  __syncthreads();
  uint32_t base = a.prev ? *a.prev : 0u, tot = 0;
  for (uint32_t k = 0; k < (uint32_t)kWaves; ++k) {
    base += before_tot[k];
    if (k < wave) base += wave_tot[k];
    tot += wave_tot[k];
  }
  gck::select_write(word, m, t, base + incl - pc, a.o);
  if (threadIdx.x == 0 && tile0 + blockDim.x >= a.words) {  // (wave 0: base holds nothing of this tile)
    const uint32_t total = base + tot;
    if (a.next) *a.next = total;
    *a.out_n = total;
  }
}

// A cross filter request (include/gck.h gck_filter_cross_device): the row-segmented selection over
// the finished row-padded plane, a request-level step behind the last tile or chunk — three kernels
// with nothing between them but the kernel boundary. k_dc_rows_count: what each row keeps, into
// row_off[s + 1] (and its survivors into row_n[s]); k_dc_rows_scan: one block turns those into the
// inclusive prefix in place; k_dc_rows_write: the kept survivors' records at row_off[s] + j.
// The lane mapping of the count and the write kernel (select_plane.hpp select_row_lanes): a row of
// `stride` words takes L lanes, L the smallest power of two >= stride within 1 .. 64, one word per
// lane; a wave carries 64 / L rows. A row of more than 64 words (the expanded path only: an in-place
// tile has R < GCK_CROSS_IDS) takes the whole wave, 64 words at a time.
struct DcRows {
  const unsigned long long* plane;
  uint32_t S, R, stride, mask, row_limit;
  uint32_t* row_off;
  uint32_t* row_n;
  gck::SelectRowsOut o;
  uint32_t* out_n;
};

static_assert(gck::kRowPiece == 64u, "a piece of a row is one word per lane of a wave");

// This lane's row and its word within a piece of it. Every lane of a wave stays in the kernel (the
// shuffles below take the whole wave): a lane beyond S or beyond the row holds an empty word.
__device__ inline void dc_row_lane(uint32_t stride, uint32_t& L, uint32_t& row, uint32_t& j) {
  L = gck::select_row_lanes(stride);
  const uint32_t lane = threadIdx.x & 63u, gw = blockIdx.x * (uint32_t)kWaves + (threadIdx.x >> 6);
  row = gw * (64u / L) + lane / L;
  j = lane & (L - 1u);
}

// Word t of `row` as its survivor mask (`word` gets the plane word); a padding lane of the row's
// last word never survives, whatever the plane holds there, so a survivor's column is below R.
__device__ inline uint64_t dc_row_word(const DcRows& a, uint32_t row, uint32_t t, uint64_t& word) {
  word = row < a.S && t < a.stride ? reinterpret_cast<const uint64_t*>(a.plane)[(size_t)row * a.stride + t] : 0ull;
  return gck::select_row_mask(word, a.mask, t, a.R);
}

__global__ void __launch_bounds__(kBlock) k_dc_rows_count(DcRows a) {
  uint32_t L, row, j;
  dc_row_lane(a.stride, L, row, j);
  uint32_t sum = 0;
  for (uint32_t p0 = 0; p0 < a.stride; p0 += gck::kRowPiece) {  // (one pass unless stride > 64; the carried count is `sum`)
    uint64_t word;
    sum += gck::select_count(dc_row_word(a, row, p0 + j, word));
  }
  for (uint32_t d = L >> 1; d >= 1u; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)d, 64);  // (d < L: inside the row's lanes)
  if (j == 0u && row < a.S) {
    a.row_off[row + 1u] = gck::select_row_kept(sum, a.row_limit);
    if (a.row_n) a.row_n[row] = sum;
  }
}

// row_off[1 .. S] (each row's kept count) into the inclusive prefix, in place: one block, a tile of
// blockDim entries at a time with a running base, as k_dc_emit scans. row_off[0] = 0 and *out_n =
// the total (below 2^32: at most S * R).
__global__ void __launch_bounds__(kBlock) k_dc_rows_scan(uint32_t* row_off, uint32_t S, uint32_t* out_n) {
  __shared__ uint32_t wave_tot[kWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t run = 0;
  for (uint32_t t0 = 0; t0 < S; t0 += blockDim.x) {
    const uint32_t t = t0 + threadIdx.x;
    uint32_t incl = t < S ? row_off[t + 1u] : 0u;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
      if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63u) wave_tot[wave] = incl;
    __syncthreads();
    uint32_t before = 0, tot = 0;
    for (uint32_t k = 0; k < (uint32_t)kWaves; ++k) {
      if (k < wave) before += wave_tot[k];
      tot += wave_tot[k];
    }
    if (t < S) row_off[t + 1u] = run + before + incl;
    run += tot;
    __syncthreads();  // (wave_tot is rewritten by the next tile)
  }
  if (threadIdx.x == 0) {
    row_off[0] = 0u;
    *out_n = run;
  }
}

__global__ void __launch_bounds__(kBlock) k_dc_rows_write(DcRows a) {
  uint32_t L, row, j;
  dc_row_lane(a.stride, L, row, j);
  const uint32_t row_base = row < a.S ? a.row_off[row] : 0u;
  uint32_t carry = 0;  // the row's survivors in the pieces before this one (the same in every lane of the row)
  for (uint32_t p0 = 0; p0 < a.stride; p0 += gck::kRowPiece) {
    const uint32_t t = p0 + j;
    uint64_t word;
    const uint64_t m = dc_row_word(a, row, t, word);
    const uint32_t pc = gck::select_count(m);
    uint32_t incl = pc;
    for (uint32_t d = 1; d < L; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
      if (j >= d) incl += up;  // (lane - d is inside the row's lanes)
    }
    gck::select_write_row(word, m, t * 32u, carry + incl - pc, row_base, a.row_limit, a.o);
    if (a.stride <= gck::kRowPiece) break;
    carry += (uint32_t)__shfl((int)incl, 63, 64);  // (L == 64: the wave is one row)
    if (a.row_limit && carry >= a.row_limit) break;  // (wave-uniform)
  }
}

// The three kernels on `st`; the caller waits. S == 0 writes row_off[0] and *out_n alone; R == 0
// (stride 0, no plane read) writes S + 1 zeros and S zero row counts.
static void dc_select_rows(const gck_select_rows& sel, const unsigned long long* plane, size_t S, size_t R,
                           const uint32_t* resources, hipStream_t st) {
  DcRows a{};
  a.plane = plane;
  a.S = (uint32_t)S;
  a.R = (uint32_t)R;
  a.stride = (uint32_t)((R + 31u) / 32u);
  a.mask = sel.mask;
  a.row_limit = sel.row_limit;
  a.row_off = sel.d_out_row_off;
  a.row_n = sel.d_out_row_n;
  a.o = gck::SelectRowsOut{sel.d_out_ids, sel.d_out_col, sel.d_out_perm, (uint32_t)std::min<size_t>(sel.cap, 0xFFFFFFFFu),
                           resources};
  a.out_n = sel.d_out_n;
  const uint32_t per_block = (uint32_t)kWaves * (64u / gck::select_row_lanes(a.stride));
  const dim3 grid((a.S + per_block - 1u) / per_block), block(kBlock);
  if (a.S) {
    hipLaunchKernelGGL(k_dc_rows_count, grid, block, 0, st, a);
    HIP_OK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_dc_rows_scan, dim3(1), block, 0, st, a.row_off, a.S, a.out_n);
  HIP_OK(hipGetLastError());
  if (a.S && a.stride && a.o.cap) {
    hipLaunchKernelGGL(k_dc_rows_write, grid, block, 0, st, a);
    HIP_OK(hipGetLastError());
  }
}

// An empty cross filter request (S == 0 or R == 0: no workspace, no check): its offsets and counts.
void device_select_rows_empty(Engine& e, const gck_select_rows& sel, size_t S, void* stream) {
  HIP_OK(hipSetDevice(e.device));
  dc_select_rows(sel, nullptr, S, 0, nullptr, (hipStream_t)stream);
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
}

// A cross filter request by resource (include/gck.h gck_filter_cross_cols_device): the mirror of the
// step above, a column-segmented selection over the same finished row-padded plane, in the same two
// places. k_dc_cols_count: what each column keeps, into col_off[r + 1] (and its survivors into
// col_n[r]); k_dc_rows_scan, as it is, over (col_off, R, out_n); k_dc_cols_write: the kept survivors'
// records at col_off[r] + j, j ascending with s.
// The mapping (select_plane.hpp): a block is kColGroup = 64 columns — the plane's word-columns
// 2 * blockIdx and 2 * blockIdx + 1 — by kColChunks = 16 waves. It takes the S rows in tiles of
// kColTile = 2,048: the tile's two words per row go to LDS by one coalesced read, all of it in
// flight at once, and every later look at the plane is an LDS read. Lane l of wave k has column
// 64 * blockIdx + l and rows [k * n, (k + 1) * n) of the tile, n = ceil(rows of the tile / 16). A
// thread counts its column in its chunk; the 16 counts of a column meet in LDS, and the chunks before
// a thread's own (and the tiles before, a running count) are its carried in-column rank. One block
// walks all S rows of its 64 columns: a plane of millions of subjects by a handful of resources (the
// expanded path only; an in-place plane is one tile) selects slowly but correctly.
struct DcCols {
  const unsigned long long* plane;
  uint32_t S, R, stride, mask, col_limit;
  uint32_t* col_off;
  uint32_t* col_n;
  gck::SelectColsOut o;
};

constexpr int kColBlock = (int)(gck::kColGroup * gck::kColChunks);
static_assert(gck::kColGroup == 64u && kColBlock <= 1024, "a column per lane, a chunk per wave, one block");

struct DcColsLds {
  uint64_t tile[gck::kColTile][2];                  // the block's two word-columns of the tile's rows
  uint32_t part[gck::kColChunks][gck::kColGroup];  // a column's survivors per chunk
};

// Rows [t0, t0 + T) of the block's two word-columns into lds.tile; a word-column beyond the row
// (stride odd, the last block) is staged as 0, which never survives. The caller's barrier follows.
__device__ inline void dc_cols_stage(const DcCols& a, DcColsLds& lds, uint32_t t0, uint32_t T) {
  const uint64_t* plane = reinterpret_cast<const uint64_t*>(a.plane);
  const uint32_t w0 = 2u * blockIdx.x;
#pragma unroll 4
  for (uint32_t i = threadIdx.x; i < 2u * T; i += (uint32_t)kColBlock) {
    const uint32_t row = i >> 1, t = w0 + (i & 1u);
    lds.tile[row][i & 1u] = t < a.stride ? plane[(size_t)(t0 + row) * a.stride + t] : 0ull;
  }
}

// This thread's chunk of a staged tile of T rows: its first row in the tile and its number of rows.
__device__ inline void dc_cols_chunk(uint32_t T, uint32_t& r0, uint32_t& n) {
  const uint32_t per = gck::select_col_chunk_rows(T);
  r0 = min(T, (threadIdx.x >> 6) * per);
  n = min(per, T - r0);
}

// Every thread of the block reaches every barrier below: a thread whose column is beyond R stages
// words as the others do, counts 0 and writes nothing.
__global__ void __launch_bounds__(kColBlock) k_dc_cols_count(DcCols a) {
  __shared__ DcColsLds lds;
  const uint32_t lane = threadIdx.x & 63u, chunk = threadIdx.x >> 6, c = blockIdx.x * gck::kColGroup + lane;
  uint32_t met = 0;
  for (uint32_t t0 = 0; t0 < a.S; t0 += min(gck::kColTile, a.S - t0)) {  // (t0 never wraps)
    const uint32_t T = min(gck::kColTile, a.S - t0);
    dc_cols_stage(a, lds, t0, T);
    __syncthreads();
    uint32_t r0, n;
    dc_cols_chunk(T, r0, n);
    met += gck::select_col_walk(&lds.tile[r0][lane >> 5], 2, a.R, a.mask, c, t0 + r0, n, nullptr, 0u, 0u, 0u);
    __syncthreads();  // (the tile is restaged)
  }
  lds.part[chunk][lane] = met;
  __syncthreads();
  if (chunk != 0u || c >= a.R) return;
  uint32_t surv = 0;
  for (uint32_t k = 0; k < gck::kColChunks; ++k) surv += lds.part[k][lane];
  a.col_off[c + 1u] = gck::select_row_kept(surv, a.col_limit);
  if (a.col_n) a.col_n[c] = surv;
}

__global__ void __launch_bounds__(kColBlock) k_dc_cols_write(DcCols a) {
  __shared__ DcColsLds lds;
  const uint32_t lane = threadIdx.x & 63u, chunk = threadIdx.x >> 6, c = blockIdx.x * gck::kColGroup + lane;
  // (read beside the first tile's words, not behind them)
  const uint32_t base = c < a.R ? a.col_off[c] : 0u, kept = c < a.R ? a.col_off[c + 1u] - base : 0u;  // (the scan's: min(surv, col_limit))
  uint32_t carry = 0;  // the column's survivors in the tiles before this one
  for (uint32_t t0 = 0; t0 < a.S; t0 += min(gck::kColTile, a.S - t0)) {
    const uint32_t T = min(gck::kColTile, a.S - t0);
    dc_cols_stage(a, lds, t0, T);
    __syncthreads();
    uint32_t r0, n;
    dc_cols_chunk(T, r0, n);
    const uint64_t* mine = &lds.tile[r0][lane >> 5];
    lds.part[chunk][lane] = gck::select_col_walk(mine, 2, a.R, a.mask, c, t0 + r0, n, nullptr, 0u, 0u, 0u);
    __syncthreads();
    uint32_t rank = carry;
    for (uint32_t k = 0; k < gck::kColChunks; ++k) {
      const uint32_t p = lds.part[k][lane];
      if (k < chunk) rank += p;
      carry += p;
    }
    if (rank < kept && base + rank < a.o.cap) gck::select_col_walk(mine, 2, a.R, a.mask, c, t0 + r0, n, &a.o, rank, base, kept);
    __syncthreads();  // (the tile and the counts are rewritten)
  }
}

// The three kernels on `st`; the caller waits. R == 0 writes col_off[0] and *out_n alone; S == 0 (no
// plane read) writes R + 1 zeros and R zero column counts.
static void dc_select_cols(const gck_select_cols& sel, const unsigned long long* plane, size_t S, size_t R,
                           const uint32_t* subjects, hipStream_t st) {
  DcCols a{};
  a.plane = plane;
  a.S = (uint32_t)S;
  a.R = (uint32_t)R;
  a.stride = (uint32_t)((R + 31u) / 32u);
  a.mask = sel.mask;
  a.col_limit = sel.col_limit;
  a.col_off = sel.d_out_col_off;
  a.col_n = sel.d_out_col_n;
  a.o = gck::SelectColsOut{sel.d_out_ids, sel.d_out_row, sel.d_out_perm, (uint32_t)std::min<size_t>(sel.cap, 0xFFFFFFFFu),
                           subjects};
  const dim3 grid((a.R + gck::kColGroup - 1u) / gck::kColGroup), block(kColBlock);
  if (a.R) {
    hipLaunchKernelGGL(k_dc_cols_count, grid, block, 0, st, a);
    HIP_OK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_dc_rows_scan, dim3(1), dim3(kBlock), 0, st, a.col_off, a.R, sel.d_out_n);
  HIP_OK(hipGetLastError());
  if (a.S && a.R && a.o.cap) {
    hipLaunchKernelGGL(k_dc_cols_write, grid, block, 0, st, a);
    HIP_OK(hipGetLastError());
  }
}

// An empty cross filter request by resource (S == 0 or R == 0: no workspace, no check).
void device_select_cols_empty(Engine& e, const gck_select_cols& sel, size_t R, void* stream) {
  HIP_OK(hipSetDevice(e.device));
  dc_select_cols(sel, nullptr, 0, R, nullptr, (hipStream_t)stream);
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
}

// A group filter request (include/gck.h gck_filter_groups_device): S owners, each with its own run
// of a flat candidate list, the runs given by S + 1 offsets in device memory. k_dc_group_check
// validates the offsets once per request (the smallest bad s into a word the host reads at the end);
// k_dc_group_pairs expands a chunk to the 8-B pairs a uniform device chunk's join reads, into the
// workspace's dc_pairs; behind the last chunk the segmented selection over the dense plane —
// k_dc_groups_count, k_dc_rows_scan as it is, k_dc_groups_write.
// Nothing has validated the offsets when these kernels read them, so each of them stays in bounds
// whatever they hold (select_plane.hpp select_group_of, select_group_range): a group index is within
// [0, S - 1], a group's range within [0, n], a record's rank below cap.

// Entry t of the S + 1 offsets against the rule off[0] == 0, off[s] <= off[s + 1], off[S] == n.
__global__ void __launch_bounds__(kBlock) k_dc_group_check(const uint32_t* off, uint32_t S, uint32_t n, uint32_t* bad) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t > S) return;
  const uint32_t v = off[t];
  const bool wrong = (t == 0u && v != 0u) || (t == S && v != n) || (t < S && v > off[t + 1u]);
  if (wrong) atomicMin(bad, t);
}

// Check pos + i of the request as a pair at pairs[i]: its group's owner and its own candidate, in
// the order the joins read a pair (resource id in the low half). The candidate load and the pair
// store are coalesced; the search reads the offsets, a few lines that stay in L2.
struct DcGroupPairs {
  const uint32_t* off;
  const uint32_t* owners;
  const uint32_t* candidates;
  unsigned long long* pairs;
  uint32_t S, pos, len, vary;
};

__global__ void __launch_bounds__(kBlock) k_dc_group_pairs(DcGroupPairs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.len) return;
  const uint32_t k = a.pos + i;  // (pos + len <= n < 2^32)
  const uint32_t own = a.owners[gck::select_group_of(a.off, a.S, k)], cand = a.candidates[k];
  const uint32_t res = a.vary == GCK_VARY_SUBJECT ? own : cand, sub = a.vary == GCK_VARY_SUBJECT ? cand : own;
  a.pairs[i] = (unsigned long long)sub << 32 | res;
}

static void dc_group_pairs(Workspace& w, const CompactReq& q, size_t pos, uint32_t len, hipStream_t st) {
  DcGroupPairs a{q.group_off, q.owners, q.ids, w.dc_pairs, (uint32_t)q.S, (uint32_t)pos, len, q.vary};
  if (len > w.max_batch) throw Error(GCK_E_DEVICE, "engine invariant violated: group chunk above max_batch");
  hipLaunchKernelGGL(k_dc_group_pairs, dim3((len + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
  HIP_OK(hipGetLastError());
}

// The offsets' check on `st`, once per request and before its chunks: w.dc_aux[4] is 0xFFFFFFFF
// afterwards, or the smallest s that breaks the rule.
static void dc_group_check(Workspace& w, const CompactReq& q, hipStream_t st) {
  HIP_OK(hipMemsetAsync(w.dc_aux + 4, 0xFF, 4, st));
  hipLaunchKernelGGL(k_dc_group_check, dim3(((uint32_t)q.S + 1u + kBlock - 1) / kBlock), dim3(kBlock), 0, st, q.group_off,
                     (uint32_t)q.S, (uint32_t)q.n, w.dc_aux + 4);
  HIP_OK(hipGetLastError());
}

static void group_offsets_error(uint32_t s, size_t S, size_t n) {
  throw Error(GCK_E_INVALID_ARGUMENT,
              "group filter request: bad group offsets at s = " + std::to_string(s) + " (off[0] == 0, off[s] <= off[s + 1] and off[" +
                  std::to_string(S) + "] == " + std::to_string(n) + " must hold)");
}

// The lane mapping of the count and the write kernel: a group takes L lanes of a wave (the host's
// choice, select_group_lanes: a power of two within 1 .. 64), one plane word per lane, and a wave
// carries 64 / L groups; a group of more than L words is walked in pieces of L words, the count or the
// rank carried from piece to piece. Every lane stays in the kernel while the shuffles run — a lane
// beyond S has an empty group — and a wave's loop runs while any of its groups has words left (a
// ballot: wave-uniform).
struct DcGroups {
  const unsigned long long* plane;
  const uint32_t* off;
  uint32_t S, n, L, mask, group_limit;
  uint32_t* row_off;
  uint32_t* row_n;
  gck::SelectRowsOut o;  // (src_ids: the candidates; col: a survivor's position k)
};

// This lane's group s, its lane j within the group, the group's range [lo, hi) and its words
// [w0, w0 + nw).
__device__ inline void dc_group_lane(const DcGroups& a, uint32_t& s, uint32_t& j, uint32_t& lo, uint32_t& hi, uint32_t& w0,
                                     uint32_t& nw) {
  const uint32_t lane = threadIdx.x & 63u, gw = blockIdx.x * (uint32_t)kWaves + (threadIdx.x >> 6);
  s = gw * (64u / a.L) + lane / a.L;
  j = lane & (a.L - 1u);
  lo = hi = 0;
  if (s < a.S) gck::select_group_range(a.off, s, a.n, lo, hi);
  w0 = lo >> 5;
  nw = hi > lo ? ((hi - 1u) >> 5) - w0 + 1u : 0u;
}

__global__ void __launch_bounds__(kBlock) k_dc_groups_count(DcGroups a) {
  uint32_t s, j, lo, hi, w0, nw;
  dc_group_lane(a, s, j, lo, hi, w0, nw);
  const uint64_t* plane = reinterpret_cast<const uint64_t*>(a.plane);
  uint32_t sum = 0;
  for (uint32_t p0 = 0; __any(p0 < nw); p0 += a.L) {  // (nw <= 2^27: p0 never wraps)
    const uint32_t t = p0 + j;
    if (t < nw) sum += gck::select_count(gck::select_group_mask(plane[w0 + t], a.mask, w0 + t, lo, hi));
  }
  for (uint32_t d = a.L >> 1; d >= 1u; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)d, 64);  // (d < L: inside the group's lanes)
  if (j == 0u && s < a.S) {
    a.row_off[s + 1u] = gck::select_row_kept(sum, a.group_limit);
    if (a.row_n) a.row_n[s] = sum;
  }
}

__global__ void __launch_bounds__(kBlock) k_dc_groups_write(DcGroups a) {
  uint32_t s, j, lo, hi, w0, nw;
  dc_group_lane(a, s, j, lo, hi, w0, nw);
  const uint64_t* plane = reinterpret_cast<const uint64_t*>(a.plane);
  const uint32_t lane = threadIdx.x & 63u, last = (lane | (a.L - 1u));  // the group's last lane
  const uint32_t base = s < a.S ? a.row_off[s] : 0u;
  uint32_t carry = 0;  // the group's survivors in the pieces before this one (the same in every lane of the group)
  for (uint32_t p0 = 0; __any(p0 < nw && !(a.group_limit && carry >= a.group_limit)); p0 += a.L) {
    const uint32_t t = p0 + j;
    const uint64_t word = t < nw ? plane[w0 + t] : 0ull;
    const uint64_t m = t < nw ? gck::select_group_mask(word, a.mask, w0 + t, lo, hi) : 0ull;
    const uint32_t pc = gck::select_count(m);
    uint32_t incl = pc;
    for (uint32_t d = 1; d < a.L; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
      if (j >= d) incl += up;  // (lane - d is inside the group's lanes)
    }
    gck::select_write_row(word, m, (w0 + t) * 32u, carry + incl - pc, base, a.group_limit, a.o);
    carry += (uint32_t)__shfl((int)incl, (int)last, 64);
  }
}

// The three kernels on `st`; the caller waits. S == 0 writes row_off[0] and *out_n alone; n == 0
// reads neither the offsets nor a plane and writes S + 1 zeros and S zero counts.
static void dc_select_groups(const gck_select_groups& sel, const unsigned long long* plane, const uint32_t* off, size_t S,
                             size_t n, const uint32_t* candidates, hipStream_t st) {
  DcGroups a{};
  a.plane = plane;
  a.off = off;
  a.S = (uint32_t)S;
  a.n = (uint32_t)n;
  a.L = gck::select_group_lanes(a.n, a.S);
  a.mask = sel.mask;
  a.group_limit = sel.group_limit;
  a.row_off = sel.d_out_row_off;
  a.row_n = sel.d_out_row_n;
  a.o = gck::SelectRowsOut{sel.d_out_ids, sel.d_out_pos, sel.d_out_perm, (uint32_t)std::min<size_t>(sel.cap, 0xFFFFFFFFu),
                           candidates};
  const uint32_t per_block = (uint32_t)kWaves * (64u / a.L);
  const dim3 grid((a.S + per_block - 1u) / per_block), block(kBlock);
  if (a.S) {
    hipLaunchKernelGGL(k_dc_groups_count, grid, block, 0, st, a);
    HIP_OK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_dc_rows_scan, dim3(1), block, 0, st, a.row_off, a.S, sel.d_out_n);
  HIP_OK(hipGetLastError());
  if (a.S && a.n && a.o.cap) {
    hipLaunchKernelGGL(k_dc_groups_write, grid, block, 0, st, a);
    HIP_OK(hipGetLastError());
  }
}

// An empty group filter request (n == 0: no workspace, no check, no offset read).
void device_select_groups_empty(Engine& e, const gck_select_groups& sel, size_t S, void* stream) {
  HIP_OK(hipSetDevice(e.device));
  dc_select_groups(sel, nullptr, nullptr, S, 0, nullptr, (hipStream_t)stream);
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
}

// A recheck request (include/gck.h gck_recheck_list_device, gck_recheck_cross_device): the selection
// over two planes — the caller's previous plane and the finished new one — a request-level step in the
// two places the row selection runs: behind the last chunk or tile of the synchronous form, and in
// device_collect of a submitted batch. The previous plane may be null (all zeros); its padding lanes,
// the caller's memory, may hold anything, so every word's mask goes through change_tail_mask or
// change_row_mask. No atomics; order by construction.
//
// Dense (k_dc_diff): k_dc_select over two words per thread. A block's first rank is the count before
// the chunk (*prev; null: 0) plus its own recount of the chunk's earlier tiles plus the scan inside the
// tile; the last tile's block writes the count so far to *next — never the word `prev` names — and to
// *out_n. A plane longer than a chunk (chunk_words, at most max_batch / 32 words: what a block may count
// again) is walked chunk by chunk on one stream, the count chained through the two words of `pair`, so
// the work stays linear in the plane.
struct DcDiff {
  const unsigned long long* old_plane;  // the chunk's words of the previous plane; null: zeros
  const unsigned long long* new_plane;
  uint32_t words, n, transitions;  // the chunk's words and checks (n <= 32 * words: the tail lanes are cleared)
  gck::ChangeOut o;
  const uint32_t* prev;
  uint32_t* next;
  uint32_t* out_n;
};

__global__ void __launch_bounds__(kBlock) k_dc_diff(DcDiff a) {
  __shared__ uint32_t before_tot[kWaves];
  __shared__ uint32_t wave_tot[kWaves];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t tile0 = blockIdx.x * blockDim.x, t = tile0 + threadIdx.x;
  const uint64_t* oldp = reinterpret_cast<const uint64_t*>(a.old_plane);
  const uint64_t* newp = reinterpret_cast<const uint64_t*>(a.new_plane);
  uint32_t mine = gck::change_count_strided(oldp, newp, threadIdx.x, tile0, blockDim.x, a.transitions, a.n);
  for (int d = 32; d >= 1; d >>= 1) mine += (uint32_t)__shfl_xor((int)mine, d, 64);
  const uint64_t nw = t < a.words ? newp[t] : 0ull, ow = t < a.words && oldp ? oldp[t] : 0ull;
  const uint64_t m = t < a.words ? gck::change_tail_mask(ow, nw, a.transitions, t, a.n) : 0ull;
  const uint32_t pc = gck::select_count(m);
  uint32_t incl = pc;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
    if (lane >= (uint32_t)d) incl += up;
  }
  if (lane == 63u) {
    wave_tot[wave] = incl;
    before_tot[wave] = mine;
  }
  __syncthreads();
  uint32_t base = a.prev ? *a.prev : 0u, tot = 0;
  for (uint32_t k = 0; k < (uint32_t)kWaves; ++k) {
    base += before_tot[k];
    if (k < wave) base += wave_tot[k];
    tot += wave_tot[k];
  }
  gck::change_write(ow, nw, m, t, base + incl - pc, a.o);
  if (threadIdx.x == 0 && tile0 + blockDim.x >= a.words) {  // (wave 0: base holds nothing of this tile)
    const uint32_t total = base + tot;
    if (a.next) *a.next = total;
    *a.out_n = total;
  }
}

// The dense diff of a plane of n checks on `st`, chunk by chunk of chunk_words words; the caller
// waits. `pair`: two device words for the chained count (needed only when the plane is more than one
// chunk). n == 0 writes *d_out_n = 0 alone.
static void dc_diff_plane(const gck_select_changes& sel, const unsigned long long* old_plane,
                          const unsigned long long* new_plane, size_t n, const uint32_t* ids, uint32_t first_id,
                          size_t chunk_words, uint32_t* pair, hipStream_t st) {
  if (n == 0) {
    HIP_OK(hipMemsetAsync(sel.d_out_n, 0, 4, st));
    return;
  }
  const size_t words = (n + 31u) / 32u, cw = std::max<size_t>(chunk_words, 1);
  if (words > cw && !pair) throw Error(GCK_E_DEVICE, "engine invariant violated: a chained diff without its count words");
  for (size_t w0 = 0, k = 0; w0 < words; w0 += cw, ++k) {
    const size_t pos = w0 * 32u;
    DcDiff a{};
    a.old_plane = old_plane ? old_plane + w0 : nullptr;
    a.new_plane = new_plane + w0;
    a.words = (uint32_t)std::min(cw, words - w0);
    a.n = (uint32_t)std::min<size_t>((size_t)a.words * 32u, n - pos);
    a.transitions = sel.transitions;
    a.o = gck::ChangeOut{sel.d_out_ids, sel.d_out_pos, sel.d_out_trans, (uint32_t)std::min<size_t>(sel.cap, 0xFFFFFFFFu),
                         ids ? ids + pos : nullptr, ids ? 0u : first_id + (uint32_t)pos, (uint32_t)pos};
    a.prev = k ? pair + ((k - 1) & 1) : nullptr;
    a.next = words > cw ? pair + (k & 1) : nullptr;
    a.out_n = sel.d_out_n;
    hipLaunchKernelGGL(k_dc_diff, dim3((a.words + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
    HIP_OK(hipGetLastError());
  }
}

// Rows (k_dc_diff_rows_count, k_dc_rows_scan as it is, k_dc_diff_rows_write): the cross plane, S rows
// of `stride` words, with the lane mapping of the row selection (dc_row_lane): a row takes L lanes, a
// wave carries 64 / L rows, a longer row is walked in 64-word pieces with a carried rank. The result is
// a CSR by row; there is no per-row limit.
struct DcDiffRows {
  const unsigned long long* old_plane;  // null: zeros
  const unsigned long long* new_plane;
  uint32_t S, R, stride, transitions;
  uint32_t* row_off;
  gck::ChangeRowsOut o;
};

// Word t of `row` as its change mask (ow / nw get the two plane words). Every lane of a wave stays
// in the kernel: a lane beyond S or beyond the row holds two empty words.
__device__ inline uint64_t dc_diff_row_word(const DcDiffRows& a, uint32_t row, uint32_t t, uint64_t& ow, uint64_t& nw) {
  const bool in = row < a.S && t < a.stride;
  const size_t at = (size_t)row * a.stride + t;
  nw = in ? reinterpret_cast<const uint64_t*>(a.new_plane)[at] : 0ull;
  ow = in && a.old_plane ? reinterpret_cast<const uint64_t*>(a.old_plane)[at] : 0ull;
  return in ? gck::change_row_mask(ow, nw, a.transitions, t, a.R) : 0ull;
}

__global__ void __launch_bounds__(kBlock) k_dc_diff_rows_count(DcDiffRows a) {
  uint32_t L, row, j;
  dc_row_lane(a.stride, L, row, j);
  uint32_t sum = 0;
  for (uint32_t p0 = 0; p0 < a.stride; p0 += gck::kRowPiece) {  // (one pass unless stride > 64; the carried count is `sum`)
    uint64_t ow, nw;
    sum += gck::select_count(dc_diff_row_word(a, row, p0 + j, ow, nw));
  }
  for (uint32_t d = L >> 1; d >= 1u; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)d, 64);  // (d < L: inside the row's lanes)
  if (j == 0u && row < a.S) a.row_off[row + 1u] = sum;
}

__global__ void __launch_bounds__(kBlock) k_dc_diff_rows_write(DcDiffRows a) {
  uint32_t L, row, j;
  dc_row_lane(a.stride, L, row, j);
  const uint32_t row_base = row < a.S ? a.row_off[row] : 0u;
  uint32_t carry = 0;  // the row's changes in the pieces before this one (the same in every lane of the row)
  for (uint32_t p0 = 0; p0 < a.stride; p0 += gck::kRowPiece) {
    const uint32_t t = p0 + j;
    uint64_t ow, nw;
    const uint64_t m = dc_diff_row_word(a, row, t, ow, nw);
    const uint32_t pc = gck::select_count(m);
    uint32_t incl = pc;
    for (uint32_t d = 1; d < L; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
      if (j >= d) incl += up;  // (lane - d is inside the row's lanes)
    }
    gck::change_write_row(ow, nw, m, t * 32u, carry + incl - pc, row_base, a.o);
    if (a.stride <= gck::kRowPiece) break;
    carry += (uint32_t)__shfl((int)incl, 63, 64);  // (L == 64: the wave is one row)
  }
}

// The three kernels on `st`; the caller waits. S == 0 writes row_off[0] and *out_n alone; R == 0
// (stride 0, no plane read) writes S + 1 zeros.
static void dc_diff_rows(const gck_select_row_changes& sel, const unsigned long long* old_plane,
                         const unsigned long long* new_plane, size_t S, size_t R, const uint32_t* resources,
                         hipStream_t st) {
  DcDiffRows a{};
  a.old_plane = old_plane;
  a.new_plane = new_plane;
  a.S = (uint32_t)S;
  a.R = (uint32_t)R;
  a.stride = (uint32_t)((R + 31u) / 32u);
  a.transitions = sel.transitions;
  a.row_off = sel.d_out_row_off;
  a.o = gck::ChangeRowsOut{sel.d_out_ids, sel.d_out_col, sel.d_out_trans, (uint32_t)std::min<size_t>(sel.cap, 0xFFFFFFFFu),
                           resources};
  const uint32_t per_block = (uint32_t)kWaves * (64u / gck::select_row_lanes(a.stride));
  const dim3 grid((a.S + per_block - 1u) / per_block), block(kBlock);
  if (a.S) {
    hipLaunchKernelGGL(k_dc_diff_rows_count, grid, block, 0, st, a);
    HIP_OK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_dc_rows_scan, dim3(1), block, 0, st, a.row_off, a.S, sel.d_out_n);
  HIP_OK(hipGetLastError());
  if (a.S && a.stride && a.o.cap) {
    hipLaunchKernelGGL(k_dc_diff_rows_write, grid, block, 0, st, a);
    HIP_OK(hipGetLastError());
  }
}

// The plane-only calls (gck_diff_planes_device, gck_diff_cross_planes_device): the selection alone,
// synchronous on `stream`. The dense form chains its count through w's pair of count words, which no
// batch uses while the caller holds the workspace, in chunks of what a batch of w would be.
void device_diff_planes(Engine& e, Workspace& w, const gck_select_changes& sel, const uint64_t* d_old,
                        const uint64_t* d_new, size_t n, const uint32_t* d_ids, uint32_t first_id, void* stream) {
  HIP_OK(hipSetDevice(e.device));
  dc_diff_plane(sel, reinterpret_cast<const unsigned long long*>(d_old), reinterpret_cast<const unsigned long long*>(d_new), n,
                d_ids, first_id, (w.max_batch & ~(size_t)31) / 32u, w.dc_aux + 2, (hipStream_t)stream);
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
}

void device_diff_rows(Engine& e, const gck_select_row_changes& sel, const uint64_t* d_old, const uint64_t* d_new,
                      size_t S, size_t R, const uint32_t* d_resources, void* stream) {
  HIP_OK(hipSetDevice(e.device));
  dc_diff_rows(sel, reinterpret_cast<const unsigned long long*>(d_old), reinterpret_cast<const unsigned long long*>(d_new), S,
               R, d_resources, (hipStream_t)stream);
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
}

// The word a device request counts its errors in, cleared on `st` before the request's first chunk:
// the caller's, or the workspace's own (which stays 0 until an emit adds to it).
// (the caller's word of a submitted batch is left to the batch: CompactRun::zero_cnt)
static uint32_t* dc_count_begin(Workspace& w, const CompactReq& q, hipStream_t st, bool shared) {
  uint32_t* cnt = q.d_n_errs ? q.d_n_errs : w.dc_aux;
  if ((q.d_n_errs && !q.zero_cnt) || (!q.d_n_errs && w.dc_cnt_dirty) || shared) HIP_OK(hipMemsetAsync(cnt, 0, 4, st));
  // (shared: the chunks on the request's other workspace add to this word too, unseen by this one)
  if (!q.d_n_errs) w.dc_cnt_dirty = shared;
  return cnt;
}

// *d_n_errs = 0 for an empty device request (no workspace, nothing else to run).
void device_zero_count(Engine& e, uint32_t* d_n_errs, void* stream) {
  if (!d_n_errs) return;
  HIP_OK(hipSetDevice(e.device));
  HIP_OK(hipMemsetAsync(d_n_errs, 0, 4, (hipStream_t)stream));
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
}

// A device request's chunk expanded to items on the device (submit_compact): the items into the
// workspace's item array on the batch's stream.
static void dc_expand(Workspace& w, const CompactReq& q, size_t pos, uint32_t len, hipStream_t st) {
  DcExpand a{};
  DcShapes t{};
  std::memcpy(t.s, q.shapes, (size_t)q.n_shapes * sizeof(gck_uniform));
  a.ids = q.cross() ? q.resources
          : q.groups() ? reinterpret_cast<const uint32_t*>(w.dc_pairs)  // (a group chunk's pairs: dc_group_pairs, before this)
          : q.list() ? (q.ids ? q.ids + pos : nullptr)
                     : q.pairs + 2 * pos;
  if (q.cross()) {
    a.subs = q.subjects;
    a.R = (uint32_t)q.R;
    a.pos = (uint32_t)pos;
  }
  a.shape_of = q.shape_of ? q.shape_of + pos : nullptr;
  a.items = w.d_items;
  a.bad = w.dc_aux + 1;
  a.n = len;
  a.n_shapes = q.n_shapes;
  a.vary = q.list() ? q.vary : 0u;
  a.fixed_id = q.fixed_id;
  a.first_id = q.first_id + (uint32_t)pos;
  if (a.shape_of) HIP_OK(hipMemsetAsync(w.dc_aux + 1, 0xFF, 4, st));
  hipLaunchKernelGGL(k_dc_expand, dim3((len + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a, t);
  HIP_OK(hipGetLastError());
  // (an engine-stream batch's join may be dispatched into the engine's HSA queue, which does not see
  // this stream's order: the items are complete before it is)
  if (st == w.stream) HIP_OK(hipStreamSynchronize(st));
}

// After a device request's batch has finished (finish_batch): the plane and the error list of its
// chunk, by kernels on the batch's stream; returns with them written. The host reads nothing but an
// expanded shaped chunk's bad-index word.
static void device_collect(Engine& e, Workspace& w) {
  (void)e;
  CompactBatch& c = w.cb;
  const uint32_t n = w.b_n;
  const uint32_t words = (n + 31u) / 32u;
  const hipStream_t st = w.b_st;
  const uint32_t cap = c.errs ? (uint32_t)std::min<size_t>(c.err_cap, 0xFFFFFFFFu) : 0u;
  bool launched = false;
  if (c.in_place()) {
    if (c.ncj) {
      hipLaunchKernelGGL(k_dc_patch, dim3((c.ncj + kBlock - 1) / kBlock), dim3(kBlock), 0, st, w.c_deferred, c.ncj, n,
                         w.d_perm, w.d_err, c.packed, w.dc_bitmap);
      HIP_OK(hipGetLastError());
      launched = true;
    }
  } else {
    if (c.indexed) {
      uint32_t bad = 0xFFFFFFFFu;
      HIP_OK(hipMemcpyAsync(&bad, w.dc_aux + 1, 4, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      if (bad != 0xFFFFFFFFu) shape_index_error(c.pos + bad, dc_shape_byte(c, bad), c.n_shapes);
    }
    if (c.cross)  // (c.out: the request's whole plane, cleared before its first chunk)
      hipLaunchKernelGGL(k_dc_cross_pack, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, w.d_perm, w.d_err, n,
                         (uint32_t)c.pos, (uint32_t)c.R, (uint32_t)((c.R + 31u) / 32u), c.out, w.dc_bitmap);
    else
      hipLaunchKernelGGL(k_dc_pack, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, w.d_perm, w.d_err, n, c.packed,
                         w.dc_bitmap);
    HIP_OK(hipGetLastError());
    launched = true;
  }
  if (launched) {
    // (a cross tile in place: c.pos is its first row's first check, and a padded index is mapped)
    const uint32_t row_len = c.grid() ? ((c.cols + 31u) / 32u) * 32u : 0u;
    hipLaunchKernelGGL(k_dc_emit, dim3(1), dim3(kBlock), 0, st, w.dc_bitmap, words, w.d_err, (uint32_t)c.pos, c.errs, cap,
                       c.d_cnt, row_len, (uint32_t)c.R);
    HIP_OK(hipGetLastError());
    if (c.d_cnt == w.dc_aux) w.dc_cnt_dirty = true;
  }
  if (c.select) {
    // the survivors of the finished plane: after the patch or the pack on this stream, for every
    // filter batch. The chunk before this one was collected — its stream completed, below — before
    // this one is, so *sel_prev holds its total
    DcSelect a{};
    a.plane = c.packed;
    a.words = words;
    a.mask = c.sel.mask;
    a.o = gck::SelectOut{c.sel.d_out_ids, c.sel.d_out_pos, c.sel.d_out_perm,
                         (uint32_t)std::min<size_t>(c.sel.cap, 0xFFFFFFFFu), c.sel_ids, c.sel_first, (uint32_t)c.pos};
    a.prev = c.sel_prev;
    a.next = c.sel_next;
    a.out_n = c.sel.d_out_n;
    hipLaunchKernelGGL(k_dc_select, dim3((words + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
    HIP_OK(hipGetLastError());
    launched = true;
  }
  if (c.select_rows) {
    // a submitted cross filter request: this batch was its one tile or chunk, so the plane is finished
    // once the kernels above have run on this stream
    dc_select_rows(c.rsel, c.out, c.rsel_S, c.R, c.rsel_ids, st);
    launched = true;
  }
  if (c.select_cols) {  // (its twin by resource: the same finished plane, by column)
    dc_select_cols(c.csel, c.out, c.csel_S, c.R, c.csel_ids, st);
    launched = true;
  }
  if (c.diff) {
    // a submitted recheck request: this batch was its one chunk, so the dense plane is finished once
    // the kernels above have run on this stream (one chunk: no chained count)
    dc_diff_plane(c.dsel, c.diff_prev, c.out, n, c.dsel_ids, c.dsel_first, words, nullptr, st);
    launched = true;
  }
  if (c.diff_rows) {  // (its cross form: this batch was the one tile or chunk of the whole plane)
    dc_diff_rows(c.rdsel, c.diff_prev, c.out, c.rdsel_S, c.R, c.rdsel_ids, st);
    launched = true;
  }
  uint32_t bad_group = 0xFFFFFFFFu;
  if (c.select_groups) {
    // a submitted group filter request: this batch was its one chunk, so the dense plane is finished;
    // the offsets' check ran on this stream before the chunk
    dc_select_groups(c.gsel, c.out, c.gsel_off, c.gsel_S, n, c.gsel_ids, st);
    HIP_OK(hipMemcpyAsync(&bad_group, w.dc_aux + 4, 4, hipMemcpyDeviceToHost, st));
    launched = true;
  }
  // (the count's clear — and the kernels above — are complete when the wait returns; a batch on the
  // caller's stream that launched nothing is ordered by that stream alone)
  if (launched || (w.b_own_stream && c.cnt_memset)) HIP_OK(hipStreamSynchronize(st));
  if (bad_group != 0xFFFFFFFFu) group_offsets_error(bad_group, c.gsel_S, n);
}
