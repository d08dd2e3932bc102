// delta.inc — Watch-driven incremental updates (included by engine.hip after bidir.inc).
//
// gck_apply_updates merges one batch of relationship updates (rel.Update: CREATE / TOUCH /
// DELETE, rel/relationship.go:267-301, as yielded by Client.UpdatesSinceRevision,
// client/client.go:370-413) into the device-resident snapshot at a new revision. The graph never
// goes back to the host:
//
//   1. host (snapshot.cpp group_updates): the updates are validated, grouped per (relation,
//      subject type, subject relation), and the last write per (object, subject) is kept;
//      CREATE and TOUCH are upserts (a Watch stream only carries committed writes), DELETE
//      removes;
//   2. device, per CSR of an affected group (plain and caveated/expiring edge classes): every
//      update key is located in its sorted row (k_delta_locate) — a key present in a class is
//      removed from it, an upsert is inserted into the class its caveat/expiration selects —
//      then the merged CSR is written in one pass: row offsets (k_delta_offsets), surviving
//      edges shifted by the updates before them (k_delta_edges), inserted edges at their merged
//      positions (k_delta_inserts). Rows stay sorted with the wildcard last, so every kernel and
//      index keeps its invariants;
//   3. the next snapshot is built (device_build in adopt mode): unchanged CSRs and their
//      indexes, and the bidirectional structures built only from unchanged CSRs, are taken over
//      without a copy; the rest is derived again from the merged arrays. Steps 2-3 run beside
//      the checks of the current snapshot (the engine lock held shared): nothing of it changes;
//   4. publish (the engine lock exclusive, milliseconds): the batches in flight finish, the
//      membership index of each merged CSR is patched in place (deleted keys become tombstones,
//      inserted keys claim empty slots; rebuilt in step 3 instead once tombstones and inserts
//      would fill 3/4 of it), and the new snapshot replaces the current one.
//
// Cost per batch: HBM-bound copies of the affected CSRs (8 B per edge of an affected plain CSR,
// 20 B per caveated one), O(updates) index patches, and the re-derivation of the transposed
// CSRs / ancestor closure whose source changed.

constexpr unsigned long long kTombKey = 0xFFFFFFFF00000000ull;  // object id 0xFFFFFFFF never exists

// Update key: (object << 32) | subject, ascending and unique per group.
__host__ __device__ __forceinline__ uint32_t dk_row(unsigned long long k) { return (uint32_t)(k >> 32); }
__host__ __device__ __forceinline__ uint32_t dk_sid(unsigned long long k) { return (uint32_t)k; }

// One CSR class of a Watch batch as the batched delta kernels see it. Every class of a batch is
// handled by the same three launches (locate, prefix, merge) whatever the number of classes: a
// block finds its class from the first-block fields (a batch touches a few dozen at most).
struct DJob {
  const uint32_t* old_off;
  const uint32_t* old_nbr;
  const uint32_t* old_cav;
  const int64_t* old_exp;
  const unsigned long long* keys;  // update keys, (object << 32) | subject, ascending
  const uint32_t* cav_in;          // caveat instance / expiration of each upsert (ext classes)
  const int64_t* exp_in;
  uint32_t* pos;                   // lower bound of each key in the old CSR
  uint8_t* found;                  // key present in the old CSR (removed)
  uint8_t* ins;                    // key inserted into this class
  uint32_t* ipre;                  // exclusive prefix counts of ins / found, D + 1 each
  uint32_t* fpre;
  uint32_t* off;                   // merged CSR (capacity: old edges + upserts of this class)
  uint32_t* nbr;
  uint32_t* cav;
  int64_t* exp;
  unsigned long long* mhash;       // membership index patched in place, or null
  unsigned long long mmask;
  uint32_t* tot;                   // [inserted, removed] after the prefix kernel
  // per k_dj_merge tile, the first key in it (k_dj_locate_prefix's atomicMin over a table uploaded
  // as kDjEmpty; null: the merge searches): rstart by row, tiles_for(n_rows + 1) + 1 entries;
  // estart by position, tiles_for(E) + 1 entries, the last for the keys at E (rows past the old ones)
  uint32_t* rstart;
  uint32_t* estart;
  uint32_t n_old, E, n_rows, D, ext;
  uint32_t l0;                     // first block of this class in k_dj_locate_prefix
  uint32_t m0[4];                  // first blocks in k_dj_merge: offsets, edges, inserts, index patch
};

__device__ __forceinline__ int dj_find(const DJob* __restrict__ jobs, int n_jobs, uint32_t b, bool merge) {
  int j = 0;
  while (j + 1 < n_jobs && (merge ? jobs[j + 1].m0[0] : jobs[j + 1].l0) <= b) ++j;
  return j;
}

constexpr int kDjScan = 1024;
constexpr uint32_t kDjTile = kBlock * 8;  // k_dj_merge's items per block (offsets, edges)
constexpr uint32_t kDjEmpty = 0xFFFFFFFFu;  // a tile no key falls in

// Inclusive block-wide sum scan over NT threads (wave64 shuffles, then the wave totals).
template <int NT = kDjScan>
__device__ __forceinline__ uint32_t dj_block_scan(uint32_t v, uint32_t* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  if (lane == 63) lds[wave] = v;
  __syncthreads();
  if (threadIdx.x < 64) {
    uint32_t w = threadIdx.x < NT / 64 ? lds[threadIdx.x] : 0u;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(w, o, 64);
      if (lane >= o) w += t;
    }
    if (threadIdx.x < NT / 64) lds[threadIdx.x] = w;
  }
  __syncthreads();
  const uint32_t r = v + (wave ? lds[wave - 1] : 0u);
  __syncthreads();  // lds is reused by the next scan
  return r;
}

// One block per class: a plain edge upserted as a plain edge again is unchanged (neither removed
// nor inserted), then the exclusive prefix counts of inserts / removals and their totals.
template <int NT>
__device__ __forceinline__ void dj_prefix_body(const DJob& J, uint32_t* lds) {
  const uint32_t D = J.D, per = (D + NT - 1) / NT;
  const uint32_t lo = min(D, threadIdx.x * per), hi = min(D, lo + per);
  uint32_t si = 0, sf = 0;
  for (uint32_t d = lo; d < hi; ++d) {
    uint8_t i = J.ins[d], f = J.found[d];
    if (!J.ext && i && f) {
      J.ins[d] = J.found[d] = 0;
      i = f = 0;
    }
    si += i;
    sf += f;
  }
  uint32_t ri = dj_block_scan<NT>(si, lds) - si, rf = dj_block_scan<NT>(sf, lds) - sf;
  for (uint32_t d = lo; d < hi; ++d) {
    J.ipre[d] = ri;
    J.fpre[d] = rf;
    ri += J.ins[d];
    rf += J.found[d];
  }
  if (threadIdx.x == NT - 1) {
    J.ipre[D] = ri;
    J.fpre[D] = rf;
    J.tot[0] = ri;
    J.tot[1] = rf;
  }
}

// The position of every update key in the old CSR (lower_bound inside its row; rows past the old
// row count sit at the end) and whether the key is present there (a plain edge upserted as a plain
// edge again is unchanged: neither removed nor inserted); each block scans its own keys' insert /
// removal flags in LDS and leaves its sums in `bsum` (2 words per block), and the last of a class's
// blocks to finish scans those sums and adds each block's base to its keys' prefixes in one
// coalesced pass — then writes the totals straight into pinned host memory, for the host's wait
// (arrive: a zeroed counter per class). (The last block had scanned every flag of the class itself,
// a thread per D / 256 consecutive keys: 27 us of the host's wait at config 5's 2,500 keys a class.)
__global__ void __launch_bounds__(kBlock) k_dj_locate_prefix(const DJob* __restrict__ jobs, int n_jobs,
                                                             unsigned* __restrict__ arrive, uint32_t* __restrict__ bsum) {
  __shared__ uint32_t lds[kBlock / 64];
  __shared__ uint32_t s_carry[2];
  __shared__ unsigned s_last;
  const int jx = dj_find(jobs, n_jobs, blockIdx.x, false);
  const DJob& J = jobs[jx];
  const uint32_t D = J.D;
  const uint32_t d = (blockIdx.x - J.l0) * kBlock + threadIdx.x;
  uint32_t i = 0, f = 0, rb = kDjEmpty, eb = kDjEmpty;
  if (d < D) {
    const unsigned long long k = J.keys[d];
    const uint32_t row = dk_row(k), sid = dk_sid(k);
    uint32_t p = J.E;
    if (J.old_off && J.E > 0 && row < J.n_old) {
      uint32_t lo = J.old_off[row], hi = J.old_off[row + 1];
      const uint32_t end = hi;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (J.old_nbr[mid] < sid) lo = mid + 1;
        else hi = mid;
      }
      p = lo;
      f = (lo < end && J.old_nbr[lo] == sid) ? 1u : 0u;
    }
    i = J.ins[d];
    if (!J.ext && i && f) {
      J.ins[d] = 0;
      i = f = 0;
    }
    J.pos[d] = p;
    J.found[d] = (uint8_t)f;
    if (J.rstart) {
      rb = row / kDjTile;
      const uint32_t ne = (J.E + kDjTile - 1u) / kDjTile;
      eb = p >= J.E ? ne : p / kDjTile;
    }
  }
  if (J.rstart) {  // the merge tiles' first keys: keys ascend, so a wave's first key of a tile is its
                   // least there — one atomic per (wave, tile), not one per key (a folder class's
                   // thousands of keys share a tile)
    const uint32_t prb = (uint32_t)__shfl_up((int)rb, 1, 64), peb = (uint32_t)__shfl_up((int)eb, 1, 64);
    const bool first = (threadIdx.x & 63u) == 0u;
    if (d < D && (first || prb != rb)) atomicMin(&J.rstart[rb], d);
    if (d < D && (first || peb != eb)) atomicMin(&J.estart[eb], d);
  }
  const uint32_t ri = dj_block_scan<kBlock>(i, lds), rf = dj_block_scan<kBlock>(f, lds);  // (inclusive)
  if (d < D) {
    J.ipre[d] = ri - i;
    J.fpre[d] = rf - f;
  }
  if (threadIdx.x == kBlock - 1) {
    bsum[2 * blockIdx.x] = ri;
    bsum[2 * blockIdx.x + 1] = rf;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();  // (release: this block's flags, prefixes and sums before its arrival)
    s_last = atomicAdd(&arrive[jx], 1u) == (D + kBlock - 1) / kBlock - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();  // (acquire: the class's other blocks' sums and prefixes)
  const uint32_t nb = (D + kBlock - 1) / kBlock;
  uint32_t* bs = bsum + 2 * J.l0;
  if (threadIdx.x == 0) s_carry[0] = s_carry[1] = 0u;
  __syncthreads();
  for (uint32_t b0 = 0; b0 < nb; b0 += kBlock) {  // block bases: exclusive, in place over the sums
    const uint32_t b = b0 + threadIdx.x;
    const uint32_t vi = b < nb ? bs[2 * b] : 0u, vf = b < nb ? bs[2 * b + 1] : 0u;
    const uint32_t ci = s_carry[0], cf = s_carry[1];
    const uint32_t si = dj_block_scan<kBlock>(vi, lds), sf = dj_block_scan<kBlock>(vf, lds);
    if (b < nb) {
      bs[2 * b] = ci + si - vi;
      bs[2 * b + 1] = cf + sf - vf;
    }
    __syncthreads();  // (every thread has read the carry)
    if (threadIdx.x == kBlock - 1) {
      s_carry[0] = ci + si;
      s_carry[1] = cf + sf;
    }
    __syncthreads();
  }
  for (uint32_t e = threadIdx.x; e < D; e += kBlock) {  // (the class's first block adds nothing)
    const uint32_t b = e / kBlock;
    if (b == 0) continue;
    J.ipre[e] += bs[2 * b];
    J.fpre[e] += bs[2 * b + 1];
  }
  if (threadIdx.x == 0) {
    J.ipre[D] = s_carry[0];
    J.fpre[D] = s_carry[1];
    J.tot[0] = s_carry[0];
    J.tot[1] = s_carry[1];
  }
}

__global__ void __launch_bounds__(kDjScan) k_dj_prefix(const DJob* __restrict__ jobs) {
  __shared__ uint32_t lds[kDjScan / 64];
  const DJob& J = jobs[blockIdx.x];
  dj_prefix_body<kDjScan>(J, lds);
}

// First index in [lo, hi) with v[i] >= x (v ascending).
template <class T, class X>
__device__ __forceinline__ uint32_t lower_idx(const T* v, uint32_t lo, uint32_t hi, X x) {
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (v[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// First index in [lo, hi) with v[i] > x.
template <class T, class X>
__device__ __forceinline__ uint32_t upper_idx(const T* v, uint32_t lo, uint32_t hi, X x) {
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (v[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The row offsets and the surviving edges are written kDjTile items per block (kDjTile / kBlock
// per thread, strided so that a wave's accesses stay contiguous): each block first finds the
// window of updates its items fall in with two binary searches over the whole update list —
// ~12 dependent reads, paid once per 2,048 items — and stages that window (a few updates at
// Watch rates) in LDS, so that each item's own search and prefix reads are LDS reads and the
// tile is one coalesced copy. A window larger than kDjWin (a dense batch) is read in place.
constexpr uint32_t kDjWin = 256;

struct DjLds {
  uint32_t win[2];
  unsigned long long key[kDjWin];  // offsets: the window's update keys
  uint32_t pos[kDjWin];            // edges: the window's update positions
  uint32_t ipre[kDjWin + 1];
  uint32_t fpre[kDjWin + 1];
  uint8_t found[kDjWin];
};

// A merge tile's window from the first-key table (wave 0): the first key of tile t or of the next
// tile holding one, and the same from t + 1 — one round of loads where two searches over the whole
// key list took ~12 dependent ones at the head of every block.
__device__ __forceinline__ void dj_window(const uint32_t* st, uint32_t t, uint32_t n, uint32_t D, uint32_t* win) {
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  uint32_t w0 = kDjEmpty, w1 = kDjEmpty;
  for (uint32_t b = t; b <= n && w1 == kDjEmpty; b += 64) {
    const uint32_t i = b + (uint32_t)lane;
    const uint32_t v = i <= n ? st[i] : kDjEmpty;
    for (unsigned long long m = __ballot(v != kDjEmpty); m; m &= m - 1ull) {  // (uniform)
      const int l = __ffsll((long long)m) - 1;
      const uint32_t x = (uint32_t)__shfl((int)v, l, 64);
      if (w0 == kDjEmpty) w0 = x;
      if (b + (uint32_t)l > t) {
        w1 = x;
        break;
      }
    }
  }
  if (lane == 0) {
    win[0] = w0 == kDjEmpty ? D : w0;
    win[1] = w1 == kDjEmpty ? D : w1;
  }
}

// new_off[r] = old_off[min(r, n_old)] + (inserts - removals) of the updates in rows < r, for
// r in [0, n_rows].
__device__ __forceinline__ void dj_offsets(const DJob& J, uint32_t blk, DjLds& L) {
  const uint32_t r0 = blk * kDjTile, r1 = min(r0 + kDjTile, J.n_rows + 1);
  if (J.rstart) {
    dj_window(J.rstart, blk, (J.n_rows + kDjTile) / kDjTile, J.D, L.win);
  } else if (threadIdx.x < 2) {
    const uint32_t r = threadIdx.x == 0 ? r0 : r1;
    L.win[threadIdx.x] = lower_idx(J.keys, 0u, J.D, (unsigned long long)r << 32);
  }
  __syncthreads();
  const uint32_t w0 = L.win[0], w1 = L.win[1], nw = w1 - w0;
  if (nw <= kDjWin) {
    for (uint32_t i = threadIdx.x; i <= nw; i += kBlock) {
      if (i < nw) L.key[i] = J.keys[w0 + i];
      L.ipre[i] = J.ipre[w0 + i];
      L.fpre[i] = J.fpre[w0 + i];
    }
    __syncthreads();
    // eight consecutive rows per thread (kDjTile = 8 kBlock): two 16-B loads and stores each, the
    // window's position advanced row to row instead of searched per row
    const uint32_t rb = r0 + threadIdx.x * 8u;
    if (rb >= r1) return;
    const bool full = rb + 8u <= r1;
    uint32_t o[8];
    if (full && J.old_off && rb + 8u <= J.n_old + 1u) {
      const u32x4 x = *reinterpret_cast<const u32x4*>(J.old_off + rb), y = *reinterpret_cast<const u32x4*>(J.old_off + rb + 4);
      o[0] = x.x, o[1] = x.y, o[2] = x.z, o[3] = x.w, o[4] = y.x, o[5] = y.y, o[6] = y.z, o[7] = y.w;
    } else {
#pragma unroll
      for (uint32_t j = 0; j < 8u; ++j) {
        const uint32_t r = rb + j;
        o[j] = r < r1 ? ((J.old_off && r <= J.n_old) ? J.old_off[r] : J.E) : 0u;
      }
    }
    uint32_t k = lower_idx(L.key, 0u, nw, (unsigned long long)rb << 32);
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
      while (k < nw && L.key[k] < ((unsigned long long)(rb + j) << 32)) ++k;
      o[j] += L.ipre[k] - L.fpre[k];
    }
    if (full) {
      *reinterpret_cast<u32x4*>(J.off + rb) = u32x4{o[0], o[1], o[2], o[3]};
      *reinterpret_cast<u32x4*>(J.off + rb + 4) = u32x4{o[4], o[5], o[6], o[7]};
    } else {
      for (uint32_t j = 0; j < 8u && rb + j < r1; ++j) J.off[rb + j] = o[j];
    }
    return;
  }
  for (uint32_t r = r0 + threadIdx.x; r < r1; r += kBlock) {
    const uint32_t k = lower_idx(J.keys, w0, w1, (unsigned long long)r << 32);
    const uint32_t base = (J.old_off && r <= J.n_old) ? J.old_off[r] : J.E;
    J.off[r] = base + J.ipre[k] - J.fpre[k];
  }
}

// Surviving old edge p moves to p + (inserts at positions <= p) - (removals at positions < p).
__device__ __forceinline__ void dj_edges(const DJob& J, uint32_t blk, DjLds& L) {
  const uint32_t p0 = blk * kDjTile, p1 = min(p0 + kDjTile, J.E);
  if (J.estart) {
    dj_window(J.estart, blk, (J.E + kDjTile - 1u) / kDjTile, J.D, L.win);
  } else if (threadIdx.x < 2) {
    L.win[threadIdx.x] = threadIdx.x == 0 ? lower_idx(J.pos, 0u, J.D, p0) : upper_idx(J.pos, 0u, J.D, p1 - 1);
  }
  __syncthreads();
  const uint32_t w0 = L.win[0], w1 = L.win[1], nw = w1 - w0;
  if (nw <= kDjWin) {
    for (uint32_t i = threadIdx.x; i <= nw; i += kBlock) {
      if (i < nw) {
        L.pos[i] = J.pos[w0 + i];
        L.found[i] = J.found[w0 + i];
      }
      L.ipre[i] = J.ipre[w0 + i];
      L.fpre[i] = J.fpre[w0 + i];
    }
    __syncthreads();
    // eight consecutive edges per thread: the old arrays read in 16-B loads, the window advanced
    // edge to edge; the stores go to their shifted positions one by one
    const uint32_t pb = p0 + threadIdx.x * 8u;
    if (pb >= p1) return;
    const bool full = pb + 8u <= p1;
    uint32_t v[8], c[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    int64_t x8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (full) {
      const u32x4 a = *reinterpret_cast<const u32x4*>(J.old_nbr + pb), b = *reinterpret_cast<const u32x4*>(J.old_nbr + pb + 4);
      v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
      if (J.ext) {
        const u32x4 ca = *reinterpret_cast<const u32x4*>(J.old_cav + pb), cb = *reinterpret_cast<const u32x4*>(J.old_cav + pb + 4);
        c[0] = ca.x, c[1] = ca.y, c[2] = ca.z, c[3] = ca.w, c[4] = cb.x, c[5] = cb.y, c[6] = cb.z, c[7] = cb.w;
#pragma unroll
        for (uint32_t j = 0; j < 8u; j += 2) {
          const u64x2 e2 = *reinterpret_cast<const u64x2*>(J.old_exp + pb + j);
          x8[j] = (int64_t)e2.x, x8[j + 1] = (int64_t)e2.y;
        }
      }
    } else {
#pragma unroll
      for (uint32_t j = 0; j < 8u; ++j) {
        const bool in = pb + j < p1;
        v[j] = in ? J.old_nbr[pb + j] : 0u;
        if (J.ext && in) {
          c[j] = J.old_cav[pb + j];
          x8[j] = J.old_exp[pb + j];
        }
      }
    }
    uint32_t l = lower_idx(L.pos, 0u, nw, pb);
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
      const uint32_t p = pb + j;
      if (p >= p1) break;
      while (l < nw && L.pos[l] < p) ++l;  // window updates at positions < p: [0, l)
      uint32_t u = l;
      bool gone = false;  // updated: removed (re-inserted if upserted here)
      while (u < nw && L.pos[u] <= p) gone |= L.found[u++] != 0;  // ... at positions <= p: [0, u)
      if (gone) continue;
      const uint32_t q = p + L.ipre[u] - L.fpre[l];
      J.nbr[q] = v[j];
      if (J.ext) {
        J.cav[q] = c[j];
        J.exp[q] = x8[j];
      }
    }
    return;
  }
  for (uint32_t p = p0 + threadIdx.x; p < p1; p += kBlock) {
    const uint32_t l = lower_idx(J.pos, w0, w1, p);
    const uint32_t u = upper_idx(J.pos, l, w1, p);
    bool gone = false;
    for (uint32_t d = l; d < u; ++d) gone |= J.found[d] != 0;
    if (gone) continue;
    const uint32_t q = p + J.ipre[u] - J.fpre[l];
    J.nbr[q] = J.old_nbr[p];
    if (J.ext) {
      J.cav[q] = J.old_cav[p];
      J.exp[q] = J.old_exp[p];
    }
  }
}

// Inserted edge d lands at pos[d] + (inserts before d) - (removals before d).
__device__ __forceinline__ void dj_inserts(const DJob& J, uint32_t d) {
  if (d >= J.D || !J.ins[d]) return;
  const uint32_t q = J.pos[d] + J.ipre[d] - J.fpre[d];
  J.nbr[q] = dk_sid(J.keys[d]);
  if (J.ext) {
    J.cav[q] = J.cav_in[d];
    J.exp[q] = J.exp_in[d];
  }
}

__device__ void dj_mhash(unsigned long long* __restrict__ tab, unsigned long long bmask,
                         const unsigned long long* __restrict__ keys, const uint8_t* __restrict__ ins,
                         const uint8_t* __restrict__ found, uint32_t D, uint32_t d);

// Everything of the merged CSRs once the prefix counts are known, one launch for all classes:
// per class the blocks of the row offsets, the surviving edges, the inserted edges and the
// membership-index patch (the old index is patched in place; nothing reads it during a batch).
__global__ void __launch_bounds__(kBlock) k_dj_merge(const DJob* __restrict__ jobs, int n_jobs) {
  __shared__ DjLds L;
  const DJob& J = jobs[dj_find(jobs, n_jobs, blockIdx.x, true)];
  const uint32_t b = blockIdx.x;
  if (b < J.m0[1]) dj_offsets(J, b - J.m0[0], L);
  else if (b < J.m0[2]) dj_edges(J, b - J.m0[1], L);
  else if (b < J.m0[3]) dj_inserts(J, (b - J.m0[2]) * kBlock + threadIdx.x);
  else dj_mhash(J.mhash, J.mmask, J.keys, J.ins, J.found, J.D, (b - J.m0[3]) * kBlock + threadIdx.x);
}

// Membership-index patch: a removed key becomes a tombstone (occupied and never matching, so
// probes of keys homed earlier still walk past it); an inserted key claims the first empty slot
// of its bucket chain (the rule bucket_probe relies on). Each bucket is read as one 64-B line (four
// 16-B loads issued together) and scanned in registers: the patch is one memory round per bucket,
// where a load per slot made it eight (config 5: 15 us for 10K keys, most of a publication). A
// plain read may miss a key another thread of this launch has just inserted: that slot then looks
// empty, the CAS on it fails and the scan goes on past it — keys are unique within a batch, so no
// other thread inserts or removes this one.
__device__ void dj_mhash(unsigned long long* __restrict__ tab, unsigned long long bmask,
                         const unsigned long long* __restrict__ keys, const uint8_t* __restrict__ ins,
                         const uint8_t* __restrict__ found, uint32_t D, uint32_t d) {
  if (d >= D || ins[d] == found[d]) return;  // presence unchanged
  const unsigned long long key = keys[d];
  unsigned long long b = mix64(key) & bmask;
  const bool remove = found[d] != 0;
  for (;;) {
    unsigned long long* bk = tab + b * kBucketKeys;
    const u64x2* p = reinterpret_cast<const u64x2*>(bk);
    const u64x2 a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3];
    const unsigned long long v[kBucketKeys] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y, a3.x, a3.y};
    bool empty = false;
    for (int k = 0; k < kBucketKeys; ++k) {
      if (v[k] == key) {
        if (remove) bk[k] = kTombKey;
        return;  // (an insert of a key already indexed: nothing to do)
      }
      if (v[k] == kEmptyKey) {
        if (remove) {
          empty = true;  // (not indexed: cannot happen for a key present in the CSR)
          break;
        }
        const unsigned long long w = atomicCAS(&bk[k], kEmptyKey, key);
        if (w == kEmptyKey || w == key) return;
      }
    }
    if (empty) return;
    b = (b + 1) & bmask;
  }
}

// ---- host side ----------------------------------------------------------------------------
//
// One Watch batch is applied with one upload, two launches and one synchronisation whatever
// the number of CSR classes it touches: every class's keys, upsert flags, caveats / expirations
// and its DJob go up in one pinned copy; k_dj_locate_prefix and k_dj_merge run for all classes at
// once; the per-class insert / removal totals are written into pinned host memory. The merged
// arrays are allocated before anything is known of the old contents, at their upper bound (old
// edges + upserts of the class); a class the batch leaves unchanged gives its copy back. Scratch
// lives in grow-only device / pinned arenas of the engine (Engine::delta_scratch, delta_host);
// only the merged CSR arrays are fresh allocations, which the next snapshot adopts.

namespace {

// Bump allocator over one byte range (256-byte aligned slices).
struct Arena {
  size_t used = 0;
  size_t take(size_t bytes) {
    const size_t at = used;
    used += (bytes + 255) & ~(size_t)255;
    return at;
  }
};

struct Job {  // one CSR class (plain or ext) of one update group
  const UpdateGroup* g;
  int ext;
  int k_old;
  uint32_t D = 0, n_cand = 0, n_rows = 0;
  bool wild_ins = false;
  size_t o_pos, o_found, o_ipre, o_fpre, o_rstart, o_estart;  // arena offsets
  DJob dj{};
};

void* arena_reserve(Engine& e, size_t bytes) {
  if (e.delta_scratch_cap < bytes) {
    if (e.delta_scratch) {  // (the last batch's index patch may still read it)
      HIP_OK(hipStreamSynchronize(nullptr));
      HIP_OK(hipFree(e.delta_scratch));
    }
    e.delta_scratch = nullptr;
    e.delta_scratch_cap = 0;
    const size_t cap = std::max(bytes + bytes / 2, (size_t)1 << 20);
    HIP_OK(hipMalloc(&e.delta_scratch, cap));
    e.delta_scratch_cap = cap;
  }
  return e.delta_scratch;
}

unsigned char* staging_reserve(Engine& e, size_t bytes) {
  if (e.delta_host_cap < bytes) {
    if (e.delta_host) HIP_OK(hipHostFree(e.delta_host));
    e.delta_host = nullptr;
    e.delta_host_cap = 0;
    const size_t cap = std::max(bytes + bytes / 2, (size_t)1 << 20);
    HIP_OK(hipHostMalloc(&e.delta_host, cap, hipHostMallocDefault));
    e.delta_host_cap = cap;
    HIP_OK(hipHostGetDevicePointer(&e.delta_host_dev, e.delta_host, 0));
  }
  return (unsigned char*)e.delta_host;
}

uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }
uint32_t tiles_for(uint64_t n) { return (uint32_t)((n + kDjTile - 1) / kDjTile); }

}  // namespace

// Subject-major keys of a batch class (for its transpose) and their source index.
__global__ void __launch_bounds__(kBlock) k_dt_swap(const unsigned long long* __restrict__ keys, uint32_t D,
                                                    unsigned long long* __restrict__ tkeys, uint32_t* __restrict__ idx) {
  const uint32_t d = blockIdx.x * kBlock + threadIdx.x;
  if (d >= D) return;
  const unsigned long long k = keys[d];
  tkeys[d] = ((unsigned long long)dk_sid(k) << 32) | dk_row(k);
  idx[d] = d;
}

// Per sorted transposed key: its insert flag and subject, and whether it changes the transpose
// (after k_dj_prefix a key inserts when ins, removes when found, and changes nothing when both are
// 0 — an upsert of a present edge or a removal of an absent one; a wildcard has no transposed row).
__global__ void __launch_bounds__(kBlock) k_dt_gather(const uint32_t* __restrict__ idx, uint32_t n,
                                                      const unsigned long long* __restrict__ tkeys,
                                                      const uint8_t* __restrict__ ins, const uint8_t* __restrict__ found,
                                                      uint32_t n_sub, uint8_t* __restrict__ ins_t,
                                                      uint32_t* __restrict__ sid_t, uint8_t* __restrict__ chg_t) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t d = idx[i], sid = (uint32_t)(tkeys[i] >> 32);
  ins_t[i] = ins[d];
  sid_t[i] = sid;
  chg_t[i] = ins[d] != found[d] && sid < n_sub ? 1u : 0u;
}

// A transposed CSR's rows are in scatter order (bidir.inc k_transpose_scatter), not ascending: a
// key's row is scanned for it (found: its position; absent: the row's end, where an insert goes),
// and the keys are then put in (row, position) order — the order k_dj_merge's prefix arithmetic
// needs (positions non-decreasing, rows ascending).
__global__ void __launch_bounds__(kBlock) k_dt_locate(const uint32_t* __restrict__ off, const uint32_t* __restrict__ nbr,
                                                      uint32_t n_old, uint32_t E, const unsigned long long* __restrict__ keys,
                                                      uint32_t D, uint32_t* __restrict__ pos, uint8_t* __restrict__ found,
                                                      unsigned long long* __restrict__ okey, uint32_t* __restrict__ idx) {
  const uint32_t d = blockIdx.x * kBlock + threadIdx.x;
  if (d >= D) return;
  const unsigned long long k = keys[d];
  const uint32_t row = dk_row(k), sid = dk_sid(k);
  uint32_t p = E, f = 0;
  if (row < n_old) {
    const uint32_t lo = off[row], hi = off[row + 1];
    p = hi;
    for (uint32_t q = lo; q < hi; ++q)
      if (nbr[q] == sid) {
        p = q;
        f = 1;
        break;
      }
  }
  pos[d] = p;
  found[d] = (uint8_t)f;
  okey[d] = ((unsigned long long)row << 32) | p;
  idx[d] = d;
}

__global__ void __launch_bounds__(kBlock) k_dt_order(const uint32_t* __restrict__ idx, uint32_t D,
                                                     const unsigned long long* __restrict__ keys,
                                                     const uint8_t* __restrict__ ins, const uint32_t* __restrict__ pos,
                                                     const uint8_t* __restrict__ found,
                                                     unsigned long long* __restrict__ keys_o, uint8_t* __restrict__ ins_o,
                                                     uint32_t* __restrict__ pos_o, uint8_t* __restrict__ found_o) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= D) return;
  const uint32_t d = idx[i];
  keys_o[i] = keys[d];
  ins_o[i] = ins[d];
  pos_o[i] = pos[d];
  found_o[i] = found[d];
}

// The transposed CSRs (subject -> objects; bidir.inc builds them for the reverse search and the
// user slots) of the plain classes the batch merged: the same update keys, subject-major, merged
// into the current snapshot's transpose by the same three kernels — about the forward merge's
// cost — instead of transposing the whole CSR again; and, per transpose, the users whose
// memberships changed (bidir.inc slots_delta recomputes only their slots). Arrays the hint needs
// until publish go to `keep`.
static void merge_transposes(Engine& e, const DeviceSnapshot& ds, const std::vector<Job>& jobs, const uint32_t* h_tot,
                             DeltaHint& hint, std::vector<void*>& fresh, std::vector<void*>& keep) {
  for (size_t i = 0; i < jobs.size(); ++i) {
    const Job& j = jobs[i];
    const DJob& J = j.dj;
    const uint32_t n_ins = h_tot[2 * i], n_rm = h_tot[2 * i + 1];
    if (j.ext || j.k_old < 0 || (n_ins == 0 && n_rm == 0)) continue;
    const DevCSR& fo = ds.table[j.k_old];
    const Derived* x = nullptr;
    for (const Derived& d : ds.derived)
      if (d.kind == 0 && d.src == fo.nbr && d.src_edges == J.E) x = &d;
    if (!x) continue;
    const UpdateGroup& g = *j.g;
    const uint32_t n_sub = e.interner[g.stype].count;
    if (n_sub != x->d.n_rows) continue;  // (new subjects: the whole transpose again)
    PhaseClock pc("transpose_delta");
    std::vector<void*> tmp;
    try {
      const uint32_t D = J.D;
      unsigned long long* tk = dalloc<unsigned long long>(tmp, D);
      unsigned long long* tks = dalloc<unsigned long long>(tmp, D);
      unsigned long long* tkc = dalloc<unsigned long long>(tmp, D);
      uint32_t* ix = dalloc<uint32_t>(tmp, D);
      uint32_t* ixs = dalloc<uint32_t>(tmp, D);
      uint8_t* ins_t = dalloc<uint8_t>(tmp, D);
      uint8_t* ins_c = dalloc<uint8_t>(tmp, D);
      uint8_t* chg_t = dalloc<uint8_t>(tmp, D);
      uint32_t* sid_t = dalloc<uint32_t>(tmp, D);
      uint32_t* sel = dalloc<uint32_t>(tmp, D);
      uint32_t* counts = dalloc<uint32_t>(tmp, 4);
      uint32_t* pos = dalloc<uint32_t>(tmp, D);
      uint8_t* fnd = dalloc<uint8_t>(tmp, D);
      uint32_t* ipre = dalloc<uint32_t>(tmp, (size_t)D + 1);
      uint32_t* fpre = dalloc<uint32_t>(tmp, (size_t)D + 1);
      uint32_t* tot = dalloc<uint32_t>(tmp, 2);
      // (k_dt_locate / k_dt_order: the compacted keys in (row, position) order)
      unsigned long long* okey = dalloc<unsigned long long>(tmp, D);
      unsigned long long* okeys = dalloc<unsigned long long>(tmp, D);
      unsigned long long* tko = dalloc<unsigned long long>(tmp, D);
      uint32_t* pos_o = dalloc<uint32_t>(tmp, D);
      uint8_t* fnd_o = dalloc<uint8_t>(tmp, D);
      uint8_t* ins_o = dalloc<uint8_t>(tmp, D);
      size_t b_sort = 0, b_flag = 0, b_flag8 = 0, b_flag64 = 0, b_uniq = 0;
      HIP_OK(hipcub::DeviceRadixSort::SortPairs(nullptr, b_sort, tk, tks, ix, ixs, (int)D, 0, 64, nullptr));
      HIP_OK(hipcub::DeviceSelect::Flagged(nullptr, b_flag, sid_t, chg_t, sel, counts, (int)D, nullptr));
      HIP_OK(hipcub::DeviceSelect::Flagged(nullptr, b_flag8, ins_t, chg_t, ins_c, counts + 2, (int)D, nullptr));
      HIP_OK(hipcub::DeviceSelect::Flagged(nullptr, b_flag64, tks, chg_t, tkc, counts + 3, (int)D, nullptr));
      HIP_OK(hipcub::DeviceSelect::Unique(nullptr, b_uniq, sel, sid_t, counts + 1, (int)D, nullptr));
      uint8_t* cub_tmp = dalloc<uint8_t>(tmp, std::max({b_sort, b_flag, b_flag8, b_flag64, b_uniq, (size_t)1}));
      HIP_OK(hipStreamSynchronize(nullptr));  // (pool allocations are ordered on the null stream)
      hipLaunchKernelGGL(k_dt_swap, dim3(blocks_for(D)), dim3(kBlock), 0, 0, J.keys, D, tk, ix);
      HIP_OK(hipcub::DeviceRadixSort::SortPairs(cub_tmp, b_sort, tk, tks, ix, ixs, (int)D, 0, 64, nullptr));
      hipLaunchKernelGGL(k_dt_gather, dim3(blocks_for(D)), dim3(kBlock), 0, 0, ixs, D, tks, J.ins, J.found, n_sub, ins_t,
                         sid_t, chg_t);
      HIP_OK(hipGetLastError());
      // only the keys that change the transpose take part in its merge
      HIP_OK(hipcub::DeviceSelect::Flagged(cub_tmp, b_flag64, tks, chg_t, tkc, counts + 3, (int)D, nullptr));
      HIP_OK(hipcub::DeviceSelect::Flagged(cub_tmp, b_flag8, ins_t, chg_t, ins_c, counts + 2, (int)D, nullptr));
      HIP_OK(hipcub::DeviceSelect::Flagged(cub_tmp, b_flag, sid_t, chg_t, sel, counts, (int)D, nullptr));
      uint32_t hc[4] = {0, 0, 0, 0}, E_t = 0;
      HIP_OK(hipMemcpy(hc, counts, 16, hipMemcpyDeviceToHost));
      const uint32_t Dc = hc[3];
      std::vector<uint8_t> h_ins(Dc);
      if (Dc) HIP_OK(hipMemcpy(h_ins.data(), ins_c, Dc, hipMemcpyDeviceToHost));
      uint32_t want_ins = 0;
      for (uint8_t v : h_ins) want_ins += v;
      HIP_OK(hipMemcpy(&E_t, x->d.off + x->d.n_rows, 4, hipMemcpyDeviceToHost));
      // the merge (one class: the forward path's kernels and block layout)
      DJob T{};
      T.old_off = x->d.off;
      T.old_nbr = x->d.nbr;
      T.keys = tko;
      T.pos = pos_o;
      T.found = fnd_o;
      T.ins = ins_o;
      T.ipre = ipre;
      T.fpre = fpre;
      T.off = ralloc<uint32_t>(e, fresh, (size_t)n_sub + 1);
      T.nbr = ralloc<uint32_t>(e, fresh, (size_t)E_t + want_ins);
      T.tot = tot;
      T.n_old = x->d.n_rows;
      T.E = E_t;
      T.n_rows = n_sub;
      T.D = Dc;
      T.ext = 0;
      T.l0 = 0;
      T.m0[0] = 0;
      T.m0[1] = tiles_for((uint64_t)n_sub + 1);
      T.m0[2] = T.m0[1] + tiles_for(E_t);
      T.m0[3] = T.m0[2] + blocks_for(Dc);
      DJob* dT = dalloc<DJob>(tmp, 1);
      HIP_OK(hipMemcpy(dT, &T, sizeof(DJob), hipMemcpyHostToDevice));
      if (Dc) {
        hipLaunchKernelGGL(k_dt_locate, dim3(blocks_for(Dc)), dim3(kBlock), 0, 0, T.old_off, T.old_nbr, T.n_old, T.E, tkc,
                           Dc, pos, fnd, okey, ix);
        HIP_OK(hipcub::DeviceRadixSort::SortPairs(cub_tmp, b_sort, okey, okeys, ix, ixs, (int)Dc, 0, 64, nullptr));
        hipLaunchKernelGGL(k_dt_order, dim3(blocks_for(Dc)), dim3(kBlock), 0, 0, ixs, Dc, tkc, ins_c, pos, fnd, tko, ins_o,
                           pos_o, fnd_o);
      }
      hipLaunchKernelGGL(k_dj_prefix, dim3(1), dim3(kDjScan), 0, 0, dT);
      hipLaunchKernelGGL(k_dj_merge, dim3(T.m0[3]), dim3(kBlock), 0, 0, dT, 1);
      HIP_OK(hipGetLastError());
      // the users the batch changed, ascending and once each
      const uint32_t n_sel = hc[0];
      HIP_OK(hipcub::DeviceSelect::Unique(cub_tmp, b_uniq, sel, sid_t, counts + 1, (int)n_sel, nullptr));
      uint32_t h_tot_t[2] = {0, 0}, n_u = 0;
      HIP_OK(hipMemcpy(&n_u, counts + 1, 4, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(h_tot_t, tot, 8, hipMemcpyDeviceToHost));
      uint32_t* ids = dalloc<uint32_t>(keep, std::max<uint32_t>(n_u, 1));
      HIP_OK(hipMemcpy(ids, sid_t, (size_t)n_u * 4, hipMemcpyDeviceToDevice));
      HIP_OK(hipDeviceSynchronize());
      // every key changes the transpose as it changed the CSR: an insert is absent from the old
      // transpose, a removal present
      if (h_tot_t[0] != want_ins || h_tot_t[1] != Dc - want_ins)
        throw Error(GCK_E_DEVICE, "engine invariant violated: transposed merge disagrees with its CSR");
      DevCSR d{};
      d.off = T.off;
      d.nbr = T.nbr;
      d.n_rows = n_sub;
      hint.derived.push_back({0, J.nbr, (uint64_t)J.E + n_ins - n_rm, d});
      hint.users.push_back({T.off, x->d.off, ids, n_u});
      if (pc.on) pc.line += " D=" + std::to_string(Dc) + " users=" + std::to_string(n_u);
    } catch (...) {
      free_list(tmp);
      throw;
    }
    free_list(tmp);
  }
}

// Builds the snapshot that grouped updates (snapshot.cpp group_updates) make of the committed one,
// without changing the committed one (steps 2-3 above); device_apply_publish swaps it in. On an
// exception the caller calls device_apply_abort.
void device_apply_build(Engine& e, const std::vector<UpdateGroup>& groups, WatchBuild& wb) {
  PhaseClock pc("apply");
  HIP_OK(hipSetDevice(e.device));
  pc.mark("setdev");
  DeviceSnapshot& ds = *e.dev;
  const Schema& sc = *e.schema;
  // the next snapshot's CSR list: every current CSR in order (adopted as is), then new classes
  std::vector<HostCSR> next(ds.base.size());
  for (size_t k = 0; k < ds.base.size(); ++k) {
    const BaseCsr& b = ds.base[k];
    const DevCSR& d = ds.table[k];
    HostCSR& h = next[k];
    h.rel = b.rel;
    h.stype = b.stype;
    h.srel = b.srel;
    h.ext = b.ext;
    h.n_rows = d.n_rows;
    h.n_edges = b.n_edges;
    h.adopt = true;
    h.dev_off = d.off;
    h.dev_nbr = d.nbr;
    h.dev_cav = d.cav;
    h.dev_exp = d.exp_us;
    h.dev_mhash = d.mhash;
    h.mmask = d.mmask;
    h.has_wild = d.has_wild;
    h.wild_known = (d.pad & kCsrWildKnown) ? 1 : 0;
    h.mh_keys = b.mh_keys;
  }
  pc.mark("next");
  // ---- host: the classes each group touches and the layout of the upload ---------------------
  // (the groups' keys, insert flags, caveats and expirations are already laid out in one pinned
  // image by group_updates — on the staging thread for a staged batch: it goes up as it is, at the
  // start of the device scratch, and only the job tables are written here)
  std::vector<Job> jobs;
  Arena ar;
  const unsigned char* img = nullptr;
  size_t img_end = 0;
  for (const UpdateGroup& g : groups) {
    if (g.keys.empty()) continue;
    if (!g.img) throw Error(GCK_E_DEVICE, "engine invariant violated: a Watch group without its upload image");
    if (img && g.img != img) throw Error(GCK_E_DEVICE, "engine invariant violated: a Watch batch over two images");
    img = g.img;
    img_end = std::max(img_end, g.o_exp + ((g.keys.size() * 8 + 255) & ~(size_t)255));
  }
  ar.take(img_end);
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    const UpdateGroup& g = groups[gi];
    const uint32_t D = (uint32_t)g.keys.size();
    if (D == 0) continue;
    for (int ext = 0; ext < 2; ++ext) {
      int k_old = -1;
      for (size_t k = 0; k < ds.base.size(); ++k)
        if (ds.base[k].rel == g.rel && ds.base[k].stype == g.stype && ds.base[k].srel == g.srel &&
            ds.base[k].ext == (ext == 1))
          k_old = (int)k;
      Job j;
      j.g = &g;
      j.ext = ext;
      j.k_old = k_old;
      j.D = D;
      j.n_cand = g.n_cand[ext];
      j.wild_ins = g.wild_ins[ext] != 0;
      if (k_old < 0 && j.n_cand == 0) continue;
      const uint32_t n_old = k_old >= 0 ? ds.table[k_old].n_rows : 0;
      j.n_rows = std::max({n_old, e.interner[sc.rels[g.rel].type].count, g.max_row[ext]});
      const uint64_t E = k_old >= 0 ? ds.base[k_old].n_edges : 0;
      if (E + j.n_cand >= 0xFFFFFFFFull) throw Error(GCK_E_CAPACITY, "a CSR would exceed 2^32-1 edges");
      jobs.push_back(std::move(j));
    }
  }
  if (jobs.empty()) return;  // (publish swaps nothing in)
  pc.mark("layout");
  const size_t o_jobs = ar.take(jobs.size() * sizeof(DJob));
  const size_t o_pjobs = ar.take(jobs.size() * sizeof(DJob));  // the deferred index patch
  const size_t o_arrive = ar.take(jobs.size() * 4);  // (k_dj_locate_prefix's counters, zeroed)
  const size_t o_win0 = ar.used;  // the merge tiles' first-key tables, uploaded as kDjEmpty
  for (Job& j : jobs) {
    const uint64_t E = j.k_old >= 0 ? ds.base[j.k_old].n_edges : 0;
    j.o_rstart = ar.take(((size_t)tiles_for((uint64_t)j.n_rows + 1) + 1) * 4);
    j.o_estart = ar.take(((size_t)tiles_for(E) + 1) * 4);
  }
  const size_t o_win1 = ar.used;
  const size_t up_end = ar.used;  // [o_jobs, up_end) goes up from the staging; the rest is device-only scratch
  const size_t o_tot = ar.take(jobs.size() * 8);
  uint32_t lb_all = 0;  // (k_dj_locate_prefix's blocks: two words of sums each)
  for (const Job& j : jobs) lb_all += blocks_for(j.D);
  const size_t o_bsum = ar.take((size_t)std::max<uint32_t>(lb_all, 1) * 8);
  for (Job& j : jobs) {
    j.o_pos = ar.take((size_t)j.D * 4);
    j.o_found = ar.take(j.D);
    j.o_ipre = ar.take(((size_t)j.D + 1) * 4);
    j.o_fpre = ar.take(((size_t)j.D + 1) * 4);
  }
  char* base = (char*)arena_reserve(e, ar.used);
  // (the host staging holds the job tables and the totals at the arena's offsets; its image
  // region stays unused)
  unsigned char* host = staging_reserve(e, o_tot + jobs.size() * 8);
  std::vector<void*>& fresh = wb.fresh;
  int64_t& tuple_delta = wb.tuple_delta;
  std::vector<DeltaHint::Fwd> fwd;  // (the merged classes, for the label tables: labels_build.inc)
  try {
    // ---- merged arrays at their upper bound, the job table, the upload -------------------------
    uint32_t lb = 0, mb = 0;
    for (Job& j : jobs) {
      const UpdateGroup& g = *j.g;
      const DevCSR* old = j.k_old >= 0 ? &ds.table[j.k_old] : nullptr;
      DJob& J = j.dj;
      J.old_off = old ? old->off : nullptr;
      J.old_nbr = old ? old->nbr : nullptr;
      J.old_cav = old ? old->cav : nullptr;
      J.old_exp = old ? old->exp_us : nullptr;
      J.keys = (const unsigned long long*)(base + g.o_keys);
      J.cav_in = j.ext ? (const uint32_t*)(base + g.o_cav) : nullptr;
      J.exp_in = j.ext ? (const int64_t*)(base + g.o_exp) : nullptr;
      J.pos = (uint32_t*)(base + j.o_pos);
      J.found = (uint8_t*)(base + j.o_found);
      J.ins = (uint8_t*)(base + g.o_ins[j.ext]);
      J.ipre = (uint32_t*)(base + j.o_ipre);
      J.fpre = (uint32_t*)(base + j.o_fpre);
      J.rstart = (uint32_t*)(base + j.o_rstart);
      J.estart = (uint32_t*)(base + j.o_estart);
    }
    pc.mark("prep");
    for (Job& j : jobs) {
      DJob& J = j.dj;
      const DevCSR* old = j.k_old >= 0 ? &ds.table[j.k_old] : nullptr;
      const uint64_t E = j.k_old >= 0 ? ds.base[j.k_old].n_edges : 0;
      const uint64_t cap = E + j.n_cand;
      J.off = ralloc<uint32_t>(e, fresh, (size_t)j.n_rows + 1);
      J.nbr = ralloc<uint32_t>(e, fresh, cap);
      if (j.ext) {
        J.cav = ralloc<uint32_t>(e, fresh, cap);
        J.exp = ralloc<int64_t>(e, fresh, cap);
      }
      // patch the index in place unless the batch could fill it past 3/4 (device_upload
      // rebuilds it then)
      if (old && old->mhash && !j.ext) {
        const uint64_t slots = (old->mmask + 1) * kBucketKeys;
        if ((ds.base[j.k_old].mh_keys + j.n_cand) * 4 <= slots * 3) {
          J.mhash = const_cast<unsigned long long*>(old->mhash);
          J.mmask = old->mmask;
        }
      }
      J.tot = (uint32_t*)((char*)e.delta_host_dev + o_tot) + 2 * (&j - jobs.data());  // (pinned: read after the wait)
      J.n_old = old ? old->n_rows : 0;
      J.E = (uint32_t)E;
      J.n_rows = j.n_rows;
      J.D = j.D;
      J.ext = (uint32_t)j.ext;
      J.l0 = lb;
      lb += blocks_for(j.D);
      J.m0[0] = mb;
      mb += tiles_for((uint64_t)j.n_rows + 1);
      J.m0[1] = mb;
      mb += tiles_for(E);
      J.m0[2] = mb;
      mb += blocks_for(j.D);
      J.m0[3] = mb;  // (the index patch runs at publish: no blocks here)
    }
    pc.mark("alloc");
    std::vector<DJob> table(jobs.size()), ptable;
    for (size_t i = 0; i < jobs.size(); ++i) table[i] = jobs[i].dj;
    // the deferred patch: the same kernel over a table of only the patch sections
    uint32_t pb = 0;
    for (const DJob& J : table)
      if (J.mhash) {
        DJob P = J;
        P.m0[0] = P.m0[1] = P.m0[2] = P.m0[3] = pb;
        pb += blocks_for(J.D);
        ptable.push_back(P);
      }
    std::memcpy(host + o_jobs, table.data(), table.size() * sizeof(DJob));
    if (!ptable.empty()) std::memcpy(host + o_pjobs, ptable.data(), ptable.size() * sizeof(DJob));
    wb.patch_jobs = base + o_pjobs;
    wb.n_patch_jobs = (int)ptable.size();
    wb.patch_blocks = pb;
    const DJob* d_jobs = (const DJob*)(base + o_jobs);
    const int n_jobs = (int)jobs.size();
    std::memset(host + o_arrive, 0, jobs.size() * 4);
    std::memset(host + o_win0, 0xFF, o_win1 - o_win0);
    uint32_t* h_tot = (uint32_t*)(host + o_tot);  // (past the uploaded range: no overlap)
    std::memset(h_tot, 0, jobs.size() * 8);
    HIP_OK(hipMemcpyAsync(base, img, img_end, hipMemcpyHostToDevice, nullptr));
    HIP_OK(hipMemcpyAsync(base + o_jobs, host + o_jobs, up_end - o_jobs, hipMemcpyHostToDevice, nullptr));
    pc.mark("upload");
    // ---- two launches; the host waits for the totals only (written by the first into pinned
    // memory), and the merge itself runs on while the next snapshot is derived: everything that
    // reads or frees the merged arrays is ordered after it on the same stream -------------------
    if (lb != lb_all) throw Error(GCK_E_DEVICE, "engine invariant violated: Watch locate blocks");
    hipLaunchKernelGGL(k_dj_locate_prefix, dim3(lb), dim3(kBlock), 0, 0, d_jobs, n_jobs, (unsigned*)(base + o_arrive),
                       (uint32_t*)(base + o_bsum));
    HIP_OK(hipEventRecord((hipEvent_t)e.delta_ev, nullptr));
    hipLaunchKernelGGL(k_dj_merge, dim3(mb), dim3(kBlock), 0, 0, d_jobs, n_jobs);
    HIP_OK(hipGetLastError());
    spin_event((hipEvent_t)e.delta_ev);
    pc.mark("merge");
    std::vector<void*> unused;
    for (size_t i = 0; i < jobs.size(); ++i) {
      Job& j = jobs[i];
      const DJob& J = j.dj;
      const uint32_t n_ins = h_tot[2 * i], n_rm = h_tot[2 * i + 1];
      if (n_ins == 0 && n_rm == 0) {  // no key of the batch changes this class
        for (const void* p : {(const void*)J.off, (const void*)J.nbr, (const void*)J.cav, (const void*)J.exp})
          if (p) unused.push_back(const_cast<void*>(p));
        continue;
      }
      tuple_delta += (int64_t)n_ins - (int64_t)n_rm;
      const UpdateGroup& g = *j.g;
      fwd.push_back({J.nbr, J.keys, J.ins, J.found, J.D, g.wild_any != 0});
      HostCSR h;
      h.rel = g.rel;
      h.stype = g.stype;
      h.srel = g.srel;
      h.ext = j.ext == 1;
      h.n_rows = j.n_rows;
      h.n_edges = (uint64_t)J.E + n_ins - n_rm;
      h.adopt = true;
      h.dev_off = J.off;
      h.dev_nbr = J.nbr;
      h.dev_cav = J.cav;
      h.dev_exp = J.exp;
      if (J.mhash) {
        h.dev_mhash = J.mhash;
        h.mmask = J.mmask;
        h.has_wild = ds.table[j.k_old].has_wild | (j.wild_ins ? 1 : 0);
        h.mh_keys = ds.base[j.k_old].mh_keys + n_ins;
      } else if (j.k_old >= 0 && (ds.table[j.k_old].pad & kCsrWildKnown)) {
        // (an index-less class: a wildcard the batch inserted sets the flag; one it removed leaves it
        // set — conservative: the planners then treat the rows as holding one)
        h.has_wild = ds.table[j.k_old].has_wild | (j.wild_ins ? 1 : 0);
        h.wild_known = 1;
      }
      if (j.k_old >= 0) next[j.k_old] = std::move(h);
      else next.push_back(std::move(h));
    }
    if (!unused.empty()) {
      fresh.erase(std::remove_if(fresh.begin(), fresh.end(),
                                 [&](void* p) { return std::find(unused.begin(), unused.end(), p) != unused.end(); }),
                  fresh.end());
      for (void* p : unused) retire_array(e, p, nullptr);
    }
  } catch (...) {
    throw;  // (device_apply_abort frees the fresh arrays)
  }
  // the transposes of the merged classes, merged too, and the users whose slots change
  DeltaHint hint;
  hint.fwd = std::move(fwd);
  std::vector<void*> keep;
  try {
    merge_transposes(e, ds, jobs, (const uint32_t*)(host + o_tot), hint, fresh, keep);
    pc.mark("transposes");
    e.delta_hint = &hint;
    wb.ds = device_build(e, next, true, wb.adopted);
    e.delta_hint = nullptr;
  } catch (...) {
    e.delta_hint = nullptr;
    free_list(keep);
    throw;
  }
  wb.ds->allocs.insert(wb.ds->allocs.end(), keep.begin(), keep.end());  // (the slot patches read them)
  pc.mark("relink");  // adopts the merged arrays and every unchanged one
}

// Step 4 (the engine lock exclusive): the batches in flight on the current snapshot finish, the
// membership indexes the new one shares with it are patched, and the new snapshot replaces it.
void device_apply_publish(Engine& e, WatchBuild& wb) {
  PhaseClock pc("apply_publish");
  HIP_OK(hipSetDevice(e.device));
  drain_batches(e);
  pc.mark("drain");
  if (!wb.ds) return;  // (no class changed)
  // the build's work on the null stream (the merge, the label tables' marks, the program upload)
  // and the membership-index patch after it are not waited for: one event behind them orders every
  // reader of the new snapshot — the launches on the engine's streams wait for it (engine.hip
  // make_ctx), dispatches into the engine's HSA queues start once it has completed (the joins'
  // aql_try), and the replaced arrays go back to the pool behind it (free_stream). (The next
  // build's host writes of the staging and program buffers come after its own wait on the null
  // stream, delta_ev, which is behind this work.)
  HIP_OK(hipEventRecord((hipEvent_t)e.build_ev, nullptr));  // (the joins wait for this one only)
  if (wb.patch_blocks) {
    hipLaunchKernelGGL(k_dj_merge, dim3(wb.patch_blocks), dim3(kBlock), 0, 0, (const DJob*)wb.patch_jobs,
                       wb.n_patch_jobs);
    HIP_OK(hipGetLastError());
  }
  HIP_OK(hipEventRecord((hipEvent_t)e.patch_ev, nullptr));
  ++e.patch_seq;
  if (e.free_stream) HIP_OK(hipStreamWaitEvent((hipStream_t)e.free_stream, (hipEvent_t)e.patch_ev, 0));
  static const bool dbg_sync_patch = debug_env("GCK_DEBUG_SYNC_PATCH") != nullptr;  // (the publication waits)
  if (dbg_sync_patch) spin_stream(e, nullptr);
  pc.mark("patch");
  {  // merged arrays the new snapshot did not take over (a transpose it no longer needs)
    std::vector<void*> a = wb.adopted;
    std::sort(a.begin(), a.end());
    for (void* p : wb.fresh)
      if (!std::binary_search(a.begin(), a.end(), p)) retire_array(e, p, nullptr);
  }
  device_publish(e, wb.ds, wb.adopted, false);  // (not waited for, above)
  wb.ds = nullptr;
  wb.fresh.clear();  // (owned by the published snapshot)
  e.n_tuples = (uint64_t)((int64_t)e.n_tuples + wb.tuple_delta);
}

// A batch that failed to build or publish: what it allocated goes back (the caller then treats the
// snapshot as lost, as a device failure may have left it half-patched).
void device_apply_abort(Engine& e, WatchBuild& wb) {
  if (wb.ds) {  // (its own arrays; what it would have taken over stays with the current snapshot)
    free_list(wb.ds->allocs);
    for (void* p : wb.ds->hallocs) (void)hipFree(p);
    delete wb.ds;
    wb.ds = nullptr;
  }
  for (void* p : wb.fresh) e.recyclable.erase(p);
  free_list(wb.fresh);  // the merged arrays
}
