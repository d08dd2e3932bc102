// bidir.inc — the reverse program behind bidirectional checks (included by engine.hip).
//
// A check (R, p, subject s) whose permission p only reaches unions of stored relations,
// computed usersets and `->` arrows (no intersection / exclusion / all(), no caveated or
// expiring edge, no wildcard subject) is a reachability question on the dispatch graph:
// vertices (object, node), an edge for every computed userset, userset tuple and arrow tuple,
// and s is reached when a vertex's row holds it directly. SpiceDB walks that graph forward from
// (R, p), depth first. When every forward path from p is shorter than the depth budget
// (checked here per node, on the snapshot's data), that walk answers HAS iff a path exists and
// NO otherwise — it can raise no depth error — so the answer is a property of the graph alone
// and any complete search gives the same bits.
//
// The bundle kernel then searches from both ends: the forward frontier from (R, p) and a
// reverse frontier from the subject over the *reverse program* built here (one reverse node
// rev(t) = n_fwd + t per forward node, whose items are t's in-edges over transposed CSRs, and
// one subject root S(type) = 2 n_fwd + type whose items are the direct-subject in-edges). Each
// level expands the smaller side (both while small); the check is HAS when the two sides claim
// a common vertex, when the forward side finds s in a row, or when the reverse side reaches
// (R, p); it is NO when either side runs out. Forward closures fan out (a group's descendants),
// reverse closures fan in (a user's ancestors), so the work of a check is bounded by the
// cheaper of the two directions instead of by the forward one.

__global__ void __launch_bounds__(kBlock) k_count_subjects(const uint32_t* __restrict__ nbr,
                                                           unsigned long long n_edges, uint32_t n_sub,
                                                           uint32_t* __restrict__ cnt) {
  const unsigned long long e = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_edges) return;
  const uint32_t x = nbr[e];
  if (x < n_sub) atomicAdd(&cnt[x], 1u);
}

// Exclusive scan of n u32 counts into out[0..n] (out[n] = total), three passes of 1024-element
// tiles: tile sums, one workgroup scanning the tile sums, then each tile's scan plus its base.
constexpr int kScanTile = 1024;

__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* sh, uint32_t& total) {
  // 1024 threads: wave scans, then a scan of the 16 wave totals
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t x = v;
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) sh[wave] = x;
  __syncthreads();
  if (threadIdx.x < 16) {
    uint32_t w = sh[threadIdx.x];
    for (int o = 1; o < 16; o <<= 1) {
      uint32_t y = __shfl_up(w, o, 16);
      if ((int)threadIdx.x >= o) w += y;
    }
    sh[16 + threadIdx.x] = w;
  }
  __syncthreads();
  total = sh[31];
  const uint32_t base = wave ? sh[16 + wave - 1] : 0u;
  __syncthreads();
  return base + x - v;
}

__global__ void __launch_bounds__(kScanTile) k_scan_tiles(const uint32_t* __restrict__ in, size_t n,
                                                          uint32_t* __restrict__ tile_sum) {
  __shared__ uint32_t sh[32];
  const size_t i = (size_t)blockIdx.x * kScanTile + threadIdx.x;
  uint32_t total;
  block_excl_scan(i < n ? in[i] : 0u, sh, total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kScanTile) k_scan_sums(uint32_t* __restrict__ s, uint32_t n) {
  __shared__ uint32_t sh[32];
  uint32_t carry = 0;
  for (uint32_t b = 0; b < n; b += kScanTile) {
    const uint32_t i = b + threadIdx.x;
    const uint32_t v = i < n ? s[i] : 0u;
    uint32_t total;
    const uint32_t x = block_excl_scan(v, sh, total);
    if (i < n) s[i] = carry + x;
    carry += total;
  }
}

__global__ void __launch_bounds__(kScanTile) k_scan_apply(const uint32_t* __restrict__ in, size_t n,
                                                          const uint32_t* __restrict__ tile_base,
                                                          uint32_t* __restrict__ out) {
  __shared__ uint32_t sh[32];
  const size_t i = (size_t)blockIdx.x * kScanTile + threadIdx.x;
  const uint32_t v = i < n ? in[i] : 0u;
  uint32_t total;
  const uint32_t x = block_excl_scan(v, sh, total);
  if (i < n) out[i] = tile_base[blockIdx.x] + x;
  if (i == n - 1) out[n] = tile_base[blockIdx.x] + x + v;
}

// Scatter every edge (row o -> subject x) into the transposed CSR (row x -> o).
__global__ void __launch_bounds__(kBlock) k_transpose_scatter(const uint32_t* __restrict__ off,
                                                              const uint32_t* __restrict__ nbr, uint32_t n_rows,
                                                              unsigned long long n_edges, uint32_t n_sub,
                                                              uint32_t* __restrict__ cursor,
                                                              uint32_t* __restrict__ nbr_t) {
  __shared__ uint32_t rows[2];
  const unsigned long long e0 = (unsigned long long)blockIdx.x * kBlock;
  const unsigned long long e = e0 + threadIdx.x;
  const uint32_t o = block_edge_row(off, n_rows, n_edges, e0, e < n_edges ? e : n_edges - 1, rows);
  if (e >= n_edges) return;
  const uint32_t x = nbr[e];
  if (x < n_sub) nbr_t[atomicAdd(&cursor[x], 1u)] = o;
}

// ---- host side ----------------------------------------------------------------------------

// Host threads for the snapshot builds: OMP_NUM_THREADS when set (a GPU box's per-GPU CPU share),
// else the hardware's, at most 16.
static unsigned host_threads() {
  static const unsigned nt = [] {
    const char* v = getenv("OMP_NUM_THREADS");
    const unsigned t = v ? (unsigned)std::max(1, atoi(v)) : std::thread::hardware_concurrency();
    return std::max(1u, std::min(t ? t : 1u, 16u));
  }();
  return nt;
}

// fn(thread, lo, hi) over [0, n) in up to `nt` contiguous chunks, on as many threads (the calling
// one included); small ranges run inline.
static void parallel_chunks(size_t n, unsigned nt, const std::function<void(unsigned, size_t, size_t)>& fn) {
  if (n < 4096 || nt <= 1) {
    if (n) fn(0, 0, n);
    return;
  }
  const size_t per = (n + nt - 1) / nt;
  std::vector<std::thread> th;
  for (unsigned t = 1; t < nt && t * per < n; ++t) th.emplace_back(fn, t, t * per, std::min(n, (t + 1) * per));
  fn(0, 0, std::min(n, per));
  for (std::thread& x : th) x.join();
}

// Topological levels of a DAG given as child lists (Kahn): `queue` holds every vertex, the levels
// one after the other (a vertex's parents all in earlier levels), level L spanning
// queue[at[L] .. at[L + 1]). False on a cycle.
struct TopoLevels {
  std::vector<uint32_t> queue;
  std::vector<size_t> at;
};

static bool topo_levels(uint32_t n, const std::vector<uint32_t>& poff, const uint32_t* coff, const uint32_t* cnbr,
                        TopoLevels& T) {
  std::vector<uint32_t> indeg(n), level(n, 0);
  std::vector<uint32_t>& queue = T.queue;
  queue.clear();
  queue.reserve(n);
  for (uint32_t y = 0; y < n; ++y) {
    indeg[y] = poff[y + 1] - poff[y];
    if (!indeg[y]) queue.push_back(y);
  }
  uint32_t max_level = 0;
  for (size_t qi = 0; qi < queue.size(); ++qi) {
    const uint32_t y = queue[qi];
    for (uint32_t k = coff[y]; k < coff[y + 1]; ++k) {
      const uint32_t c = cnbr[k];
      if (c >= n) continue;
      level[c] = std::max(level[c], level[y] + 1u);
      max_level = std::max(max_level, level[c]);
      if (--indeg[c] == 0) queue.push_back(c);
    }
  }
  if (queue.size() != n) return false;
  // by level, Kahn's order within a level (a counting sort)
  std::vector<size_t> cnt((size_t)max_level + 2, 0);
  for (uint32_t y = 0; y < n; ++y) ++cnt[level[y] + 1];
  for (size_t L = 1; L < cnt.size(); ++L) cnt[L] += cnt[L - 1];
  T.at = cnt;
  std::vector<uint32_t> by(n);
  for (uint32_t y : queue) by[cnt[level[y]]++] = y;
  queue.swap(by);
  return true;
}

// Per level of T, in parallel over the level's vertices: `make(y, scratch)` builds y's list from
// what earlier levels hold (false: y overflows, len[y] = kNone), and the level's lists are appended
// to `data` (begin[y], len[y]). False when `data` would exceed `limit`.
static bool level_lists(const TopoLevels& T, unsigned nt, std::vector<uint32_t>& data, std::vector<uint64_t>& begin,
                        std::vector<uint32_t>& len, const std::function<bool(uint32_t, std::vector<uint32_t>&)>& make,
                        uint64_t limit) {
  std::vector<std::vector<uint32_t>> buf(nt);
  std::vector<std::vector<std::pair<uint32_t, uint64_t>>> where(nt);  // (vertex, offset in its thread's buffer)
  for (size_t L = 0; L + 1 < T.at.size(); ++L) {
    const size_t b = T.at[L], e_ = T.at[L + 1];
    for (unsigned t = 0; t < nt; ++t) buf[t].clear(), where[t].clear();
    parallel_chunks(e_ - b, nt, [&](unsigned t, size_t lo, size_t hi) {
      std::vector<uint32_t> tmp;
      for (size_t k = b + lo; k < b + hi; ++k) {
        const uint32_t y = T.queue[k];
        tmp.clear();
        if (!make(y, tmp)) {
          len[y] = kNone;
          continue;
        }
        where[t].emplace_back(y, buf[t].size());
        buf[t].insert(buf[t].end(), tmp.begin(), tmp.end());
      }
    });
    size_t add = 0;
    std::vector<size_t> base(nt);
    for (unsigned t = 0; t < nt; ++t) base[t] = data.size() + add, add += buf[t].size();
    if (data.size() + add > limit) return false;
    if (data.capacity() < data.size() + add) data.reserve(std::max(2 * data.capacity(), data.size() + add));
    data.resize(data.size() + add);
    // each thread's lists go in thread order (the queue order within the level), copied in parallel
    std::vector<std::thread> th;
    auto place = [&](unsigned t) {
      for (size_t j = 0; j < where[t].size(); ++j) {
        const uint32_t y = where[t][j].first;
        const uint64_t o = where[t][j].second, o2 = j + 1 < where[t].size() ? where[t][j + 1].second : buf[t].size();
        begin[y] = base[t] + o;
        len[y] = (uint32_t)(o2 - o);
      }
      std::copy(buf[t].begin(), buf[t].end(), data.begin() + base[t]);
    };
    if (add >= 65536 && nt > 1) {
      for (unsigned t = 1; t < nt; ++t) th.emplace_back(place, t);
      place(0);
      for (std::thread& x : th) x.join();
    } else {
      for (unsigned t = 0; t < nt; ++t) place(t);
    }
  }
  return true;
}

// Tree labels and covers of a DAG (parents per vertex poff / pnbr, levels T): a spanning forest
// over each vertex's first parent, lab[2v] = pre(v) | overflow << 31, lab[2v + 1] = end(v) (x is a
// tree ancestor of y, or y, iff pre(x) <= pre(y) < end(x)), and per vertex the pruned cover
// C(y) = {y} + the covers of its parents minus every entry that is a tree ancestor of another
// (cov_off / cov_pre: preorder numbers, ascending); a vertex whose cover exceeds cover_max (or a
// parent's did) overflows and has none. Subtree sizes bottom-up, preorder numbers top-down and
// covers parents first, level by level in parallel: the preorder of a depth-first walk from the
// roots in id order, each vertex's children in id order.
static void tree_labels(uint32_t n, const std::vector<uint32_t>& poff, const std::vector<uint32_t>& pnbr,
                        const TopoLevels& T, uint32_t cover_max, unsigned nt, std::vector<uint32_t>& lab,
                        std::vector<uint32_t>& cov_off, std::vector<uint32_t>& cov_pre) {
  std::vector<uint32_t> coff((size_t)n + 1, 0), kids(n), pre(n), size(n, 1);
  for (uint32_t y = 0; y < n; ++y)
    if (poff[y + 1] > poff[y]) ++coff[pnbr[poff[y]] + 1];
  for (uint32_t y = 0; y < n; ++y) coff[y + 1] += coff[y];
  {
    std::vector<uint32_t> at(coff.begin(), coff.end() - 1);
    for (uint32_t y = 0; y < n; ++y)
      if (poff[y + 1] > poff[y]) kids[at[pnbr[poff[y]]]++] = y;
  }
  for (size_t L = T.at.size() - 1; L-- > 0;)
    parallel_chunks(T.at[L + 1] - T.at[L], nt, [&](unsigned, size_t lo, size_t hi) {
      for (size_t k = T.at[L] + lo; k < T.at[L] + hi; ++k) {
        const uint32_t y = T.queue[k];
        uint32_t sz = 1;
        for (uint32_t j = coff[y]; j < coff[y + 1]; ++j) sz += size[kids[j]];
        size[y] = sz;
      }
    });
  uint32_t next = 0;
  for (uint32_t y = 0; y < n; ++y)
    if (poff[y + 1] == poff[y]) pre[y] = next, next += size[y];
  for (size_t L = 0; L + 1 < T.at.size(); ++L)
    parallel_chunks(T.at[L + 1] - T.at[L], nt, [&](unsigned, size_t lo, size_t hi) {
      for (size_t k = T.at[L] + lo; k < T.at[L] + hi; ++k) {
        const uint32_t y = T.queue[k];
        uint32_t nx = pre[y] + 1;
        for (uint32_t j = coff[y]; j < coff[y + 1]; ++j) pre[kids[j]] = nx, nx += size[kids[j]];
      }
    });
  std::vector<uint32_t> size_at(n);  // subtree size by preorder number
  for (uint32_t y = 0; y < n; ++y) size_at[pre[y]] = size[y];
  std::vector<uint32_t> cdata;
  std::vector<uint64_t> cb(n, 0);
  std::vector<uint32_t> cl(n, 0);
  (void)level_lists(
      T, nt, cdata, cb, cl,
      [&](uint32_t y, std::vector<uint32_t>& cand) {
        cand.assign(1, pre[y]);
        for (uint32_t k = poff[y]; k < poff[y + 1]; ++k) {
          const uint32_t q = pnbr[k];
          if (cl[q] == kNone) return false;
          cand.insert(cand.end(), cdata.begin() + cb[q], cdata.begin() + cb[q] + cl[q]);
        }
        if (cand.size() > 64 * (size_t)cover_max) return false;  // (bounds the work per vertex)
        std::sort(cand.begin(), cand.end());
        cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
        // in preorder, an entry is a tree ancestor of another iff the next one lies in its subtree
        // (the entries are preorder numbers)
        size_t m = 0;
        for (size_t i = 0; i < cand.size(); ++i)
          if (!(i + 1 < cand.size() && cand[i + 1] < cand[i] + size_at[cand[i]])) cand[m++] = cand[i];
        cand.resize(m);
        return m <= cover_max;
      },
      ~0ull);
  lab.assign(2 * (size_t)n, 0);
  cov_off.assign((size_t)n + 1, 0);
  for (uint32_t y = 0; y < n; ++y) {
    const bool over = cl[y] == kNone;
    lab[2 * (size_t)y] = pre[y] | (over ? 0x80000000u : 0u);
    lab[2 * (size_t)y + 1] = pre[y] + size[y];
    cov_off[y + 1] = cov_off[y] + (over ? 0u : cl[y]);
  }
  cov_pre.resize(cov_off[n]);
  parallel_chunks(n, nt, [&](unsigned, size_t lo, size_t hi) {
    for (size_t y = lo; y < hi; ++y)
      std::copy(cdata.begin() + cb[y], cdata.begin() + cb[y] + (cov_off[y + 1] - cov_off[y]), cov_pre.begin() + cov_off[y]);
  });
}

// Exclusive scan (device) of cnt[0..n) into out[0..n].
static void device_excl_scan(const uint32_t* cnt, size_t n, uint32_t* out) {
  const size_t tiles = (n + kScanTile - 1) / kScanTile;
  std::vector<void*> tmp;
  uint32_t* sums = dalloc<uint32_t>(tmp, tiles);
  try {
    if (n == 0) {
      HIP_OK(hipMemset(out, 0, sizeof(uint32_t)));
    } else {
      hipLaunchKernelGGL(k_scan_tiles, dim3((uint32_t)tiles), dim3(kScanTile), 0, 0, cnt, n, sums);
      hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(kScanTile), 0, 0, sums, (uint32_t)tiles);
      hipLaunchKernelGGL(k_scan_apply, dim3((uint32_t)tiles), dim3(kScanTile), 0, 0, cnt, n, sums, out);
      HIP_OK(hipGetLastError());
      HIP_OK(hipDeviceSynchronize());
    }
  } catch (...) {
    free_list(tmp);
    throw;
  }
  free_list(tmp);
}

// Ancestor closure of a self-recursive userset CSR `r` (row x lists y: x#n@y#n, so x is a parent
// of y): row y of the result lists every object that reaches y through those edges, y excluded
// (Zanzibar's Leopard index, for the reverse side only). Built on the host in topological order
// (a row merges its parents' rows); returns the table index, or kNone when the data is cyclic or
// the closure would exceed 64 entries per row + edge.
// A derived structure of the previous snapshot built from the same (unchanged) source CSR, or
// nullptr. Its arrays are handed over to the new snapshot through `adopted` (device_upload).
static const Derived* reuse_derived(const Engine& e, uint8_t kind, const DevCSR& src, uint64_t ne,
                                    std::vector<void*>& adopted) {
  if (e.delta_hint)  // a transpose the Watch batch merged (delta.inc)
    for (const Derived& x : e.delta_hint->derived) {
      if (x.kind != kind || x.src != src.nbr || x.src_edges != ne) continue;
      for (const void* p : {(const void*)x.d.off, (const void*)x.d.nbr})
        if (p) adopted.push_back(const_cast<void*>(p));
      return &x;
    }
  if (!e.dev) return nullptr;
  for (const Derived& x : e.dev->derived) {
    if (x.kind != kind || x.src != src.nbr || x.src_edges != ne) continue;
    for (const void* p : {(const void*)x.d.off, (const void*)x.d.nbr, (const void*)x.d.mhash, (const void*)x.sig,
                          (const void*)x.lab, (const void*)x.cov_off, (const void*)x.cov_pre})
      if (p) adopted.push_back(const_cast<void*>(p));
    return &x;
  }
  return nullptr;
}

#include "ancestors.inc"

static uint32_t build_ancestors(Engine& e, DeviceSnapshot& ds, std::vector<DevCSR>& table, const DevCSR r,
                                uint64_t ne, std::vector<void*>& adopted) {
  if (const Derived* x = reuse_derived(e, 1, r, ne, adopted)) {
    ds.derived.push_back(*x);
    table.push_back(x->d);
    return (uint32_t)table.size() - 1;
  }
  const uint32_t n = r.n_rows;
  {  // on the device (ancestors.inc); a cyclic or oversized hierarchy falls to the host build below
    AncDevice ad;
    const uint64_t cap_d = std::min<uint64_t>(0x7FFFFFFFull, 64ull * ((uint64_t)n + ne) + 1024);
    if (build_ancestors_device(ds, r, ne, cap_d, ad)) {
      PhaseClock pc("ancestors_index");
      DevCSR d{};
      d.off = ad.aoff;
      d.nbr = ad.anbr;
      d.n_rows = n;
      if (ad.n_anc) build_mhash(ds, d, ad.n_anc);
      uint32_t* sig = dalloc<uint32_t>(ds.allocs, (size_t)n * kSigWords, &ds.bytes);
      HIP_OK(hipMemsetAsync(sig, 0, (size_t)std::max<uint32_t>(n, 1) * kSigWords * 4, nullptr));
      if (n) hipLaunchKernelGGL(k_sig_build, dim3(grid_for((unsigned long long)ad.n_anc + n)), dim3(kBlock), 0, 0, ad.aoff,
                                ad.anbr, n, (unsigned long long)ad.n_anc, sig);
      HIP_OK(hipGetLastError());
      HIP_OK(hipDeviceSynchronize());
      table.push_back(d);
      Derived x{1, r.nbr, ne, d};
      x.sig = sig;
      x.lab = ad.lab;
      x.cov_off = ad.cov_off;
      x.cov_pre = ad.cov_pre;
      ds.derived.push_back(x);
      return (uint32_t)table.size() - 1;
    }
  }
  PhaseClock pc("ancestors");
  std::vector<uint32_t> off((size_t)n + 1), nbr(ne);
  HIP_OK(hipMemcpy(off.data(), r.off, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost));
  if (ne) HIP_OK(hipMemcpy(nbr.data(), r.nbr, ne * 4, hipMemcpyDeviceToHost));
  pc.mark("download");
  std::vector<uint32_t> poff((size_t)n + 2, 0), pnbr(ne);  // parents of each row
  for (uint64_t k = 0; k < ne; ++k)
    if (nbr[k] < n) ++poff[(size_t)nbr[k] + 2];
  for (size_t y = 2; y < poff.size(); ++y) poff[y] += poff[y - 1];
  for (uint32_t x = 0; x < n; ++x)
    for (uint32_t k = off[x]; k < off[x + 1]; ++k)
      if (nbr[k] < n) pnbr[poff[(size_t)nbr[k] + 1]++] = x;
  // poff[y] .. poff[y + 1] now spans the parents of y
  const uint64_t cap = std::min<uint64_t>(0x7FFFFFFFull, 64ull * ((uint64_t)n + ne) + 1024);
  // topological levels: a row's parents all sit in earlier levels, so the rows of one level are
  // built in parallel from what the earlier levels hold (host_threads() host threads)
  TopoLevels T;
  if (!topo_levels(n, poff, off.data(), nbr.data(), T)) return kNone;  // a cycle
  const unsigned nt = host_threads();
  std::vector<uint32_t> data;
  std::vector<uint64_t> begin(n, 0);
  std::vector<uint32_t> len(n, 0);
  const bool closed = level_lists(
      T, nt, data, begin, len,
      [&](uint32_t y, std::vector<uint32_t>& tmp) {
        for (uint32_t k = poff[y]; k < poff[y + 1]; ++k) {
          const uint32_t p = pnbr[k];
          tmp.push_back(p);
          tmp.insert(tmp.end(), data.begin() + begin[p], data.begin() + begin[p] + len[p]);
        }
        if (tmp.size() > 1) {  // (rows ascending, as every CSR)
          std::sort(tmp.begin(), tmp.end());
          tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
        }
        return true;
      },
      cap);
  if (!closed) return kNone;
  pc.mark("closure");
  std::vector<uint32_t> aoff((size_t)n + 1, 0), anbr(data.size());
  for (uint32_t y = 0; y < n; ++y) aoff[y + 1] = aoff[y] + len[y];
  parallel_chunks(n, nt, [&](unsigned, size_t lo, size_t hi) {
    for (size_t y = lo; y < hi; ++y) std::copy(data.begin() + begin[y], data.begin() + begin[y] + len[y], anbr.begin() + aoff[y]);
  });
  DevCSR d{};
  uint32_t* doff = dalloc<uint32_t>(ds.allocs, (size_t)n + 1, &ds.bytes);
  uint32_t* dnbr = dalloc<uint32_t>(ds.allocs, anbr.size(), &ds.bytes);
  HIP_OK(hipMemcpy(doff, aoff.data(), aoff.size() * 4, hipMemcpyHostToDevice));
  if (!anbr.empty()) HIP_OK(hipMemcpy(dnbr, anbr.data(), anbr.size() * 4, hipMemcpyHostToDevice));
  d.off = doff;
  d.nbr = dnbr;
  d.n_rows = n;
  // "is v an ancestor of y" in one probe: lets a check whose resource lists a few groups test
  // them against a user's groups' closures without enumerating the closures
  if (!anbr.empty()) build_mhash(ds, d, anbr.size());
  // and a 256-bit signature of {y} + anc(y) per row, so that the closure-join stage probes only
  // the (group, id) pairs the signature does not rule out
  uint32_t* sig = dalloc<uint32_t>(ds.allocs, (size_t)n * kSigWords, &ds.bytes);
  HIP_OK(hipMemsetAsync(sig, 0, (size_t)std::max<uint32_t>(n, 1) * kSigWords * 4, nullptr));
  if (n) hipLaunchKernelGGL(k_sig_build, dim3(grid_for((unsigned long long)anbr.size() + n)), dim3(kBlock), 0, 0, doff,
                            dnbr, n, (unsigned long long)anbr.size(), sig);
  HIP_OK(hipGetLastError());
  pc.mark("closure_index");
  // the slot fast path's tree labels and covers (closure.inc): a spanning forest over each row's
  // first parent, preorder intervals, and per row the pruned cover C(y) = {y} + the covers of its
  // parents, minus every entry that is a tree ancestor of another
  std::vector<uint32_t> lab, cov_off, cov_pre;
  tree_labels(n, poff, pnbr, T, kCoverMax, nt, lab, cov_off, cov_pre);
  pc.mark("labels_covers");
  uint32_t* dlab = dalloc<uint32_t>(ds.allocs, std::max<size_t>(2 * (size_t)n, 1), &ds.bytes);
  uint32_t* dcoff = dalloc<uint32_t>(ds.allocs, (size_t)n + 1, &ds.bytes);
  uint32_t* dcpre = dalloc<uint32_t>(ds.allocs, std::max<size_t>(cov_pre.size(), 1), &ds.bytes);
  HIP_OK(hipStreamSynchronize(nullptr));  // the allocations are ordered on the null stream
  if (n) HIP_OK(hipMemcpy(dlab, lab.data(), lab.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dcoff, cov_off.data(), cov_off.size() * 4, hipMemcpyHostToDevice));
  if (!cov_pre.empty()) HIP_OK(hipMemcpy(dcpre, cov_pre.data(), cov_pre.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipDeviceSynchronize());
  pc.mark("upload");
  table.push_back(d);
  Derived x{1, r.nbr, ne, d};
  x.sig = sig;
  x.lab = dlab;
  x.cov_off = dcoff;
  x.cov_pre = dcpre;
  ds.derived.push_back(x);
  return (uint32_t)table.size() - 1;
}

// The slot fast path's slots over one CSR (closure.inc): user slots (kUSlotWords) over a
// transposed direct-member CSR, resource slots (kDSlotWords) over a resource's group CSR; built
// once per source per snapshot, and only while they take at most half of the free HBM.
enum class SlotKind { kUser, kResource };

// An array for the slot fast path: physically contiguous when the driver can (fewer, larger
// translations for a table read at random by every check), else from the pool.
static uint32_t* slot_alloc(DeviceSnapshot& ds, size_t bytes) {
  void* p = nullptr;
  if (hipExtMallocWithFlags(&p, std::max<size_t>(bytes, 4), hipDeviceMallocContiguous) == hipSuccess) {
    ds.hallocs.push_back(p);
    ds.bytes += bytes;
    return static_cast<uint32_t*>(p);
  }
  (void)hipGetLastError();
  uint32_t* s = dalloc<uint32_t>(ds.allocs, std::max<size_t>(bytes / 4, 1), &ds.bytes);
  HIP_OK(hipStreamSynchronize(nullptr));  // pool allocations are ordered on the null stream
  return s;
}

struct SlotSet {
  const uint32_t* slots = nullptr;
  const uint32_t* list = nullptr;  // user slots: the cover lists (null: none)
  // resource slots: their 16-B fronts (slot_pack.hpp), in the slots' own allocation behind the last
  // slot — built, adopted and freed with them, so a Watch batch that rewrites a resource's slot
  // (the whole array is rebuilt then) publishes its front with it
  const uint32_t* fronts(uint32_t n_rows) const { return slots ? slots + (size_t)n_rows * kDSlotWords : nullptr; }
};

// closure.inc k_user_slots_1p / k_user_slots_ids at the snapshot's entry width, on the null stream.
static void launch_user_slots_ids(uint32_t bits, const uint32_t* off, const uint32_t* nbr, const uint32_t* ids, uint32_t n,
                                  const uint32_t* lab, const uint32_t* cov_off, const uint32_t* cov_pre, uint32_t n_groups,
                                  const uint32_t* list_off, uint32_t* list, uint32_t* staged) {
  hipLaunchKernelGGL(bits == 24 ? k_user_slots_ids<24> : k_user_slots_ids<32>, dim3(grid_for(n)), dim3(kBlock), 0, 0, off,
                     nbr, ids, n, lab, cov_off, cov_pre, n_groups, list_off, list, staged);
  HIP_OK(hipGetLastError());
}

static void launch_user_slots_1p(uint32_t bits, const uint32_t* off, const uint32_t* nbr, uint32_t n, const uint32_t* lab,
                                 const uint32_t* cov_off, const uint32_t* cov_pre, uint32_t n_groups, uint32_t* slots,
                                 uint32_t* len) {
  hipLaunchKernelGGL(bits == 24 ? k_user_slots_1p<24> : k_user_slots_1p<32>, dim3(grid_for(n)), dim3(kBlock), 0, 0, off, nbr,
                     n, lab, cov_off, cov_pre, n_groups, slots, len);
  HIP_OK(hipGetLastError());
}

// The full build of the slots of users [0, n) into `slots`: one pass of the random reads (labels,
// covers) for every user writes the inline slots and the lengths of the lists of the users whose
// covers exceed a slot; those lists follow at the scanned offsets. alloc_list(bytes) gives the list
// array, or declines with null: the listed users then overflow. Returns the list array, and the
// lists' total length whether or not they were written.
struct UserLists {
  uint32_t* list;
  uint32_t total;
};

template <class AllocList>
static UserLists build_user_slots(uint32_t bits, const uint32_t* off, const uint32_t* nbr, uint32_t n, const uint32_t* lab,
                                  const uint32_t* cov_off, const uint32_t* cov_pre, uint32_t n_groups, uint32_t* slots,
                                  AllocList alloc_list) {
  UserLists out{nullptr, 0u};
  std::vector<void*> tmp;
  try {
    uint32_t* len = dalloc<uint32_t>(tmp, (size_t)n + 1);
    uint32_t* loff = dalloc<uint32_t>(tmp, (size_t)n + 1);
    HIP_OK(hipStreamSynchronize(nullptr));
    launch_user_slots_1p(bits, off, nbr, n, lab, cov_off, cov_pre, n_groups, slots, len);
    device_excl_scan(len, n, loff);
    HIP_OK(hipMemcpy(&out.total, loff + n, 4, hipMemcpyDeviceToHost));
    // (u32 offsets; a total that wrapped cannot be told apart, so stay well below 2^31)
    if (out.total > 0 && out.total < (1u << 31)) out.list = alloc_list((size_t)out.total * 4);
    if (out.total) {
      hipLaunchKernelGGL(bits == 24 ? k_user_lists<24> : k_user_lists<32>, dim3(grid_for(n)), dim3(kBlock), 0, 0, off, nbr, n, cov_off, cov_pre, len, loff,
                         out.list, slots);
      HIP_OK(hipGetLastError());
    }
    HIP_OK(hipDeviceSynchronize());
  } catch (...) {
    free_list(tmp);
    throw;
  }
  free_list(tmp);
  return out;
}

// A Watch batch whose hierarchy labels are unchanged recomputes the user slots of the users it
// touched only (DeltaHint::Users): their slots are staged, the rest of the current snapshot's slot
// array is taken over and the staged ones are written into it at publish (SlotPatch); their cover
// lists go after a copy of the current lists. Null when the batch gives no such case.
static const SlotSet* slots_delta(Engine& e, DeviceSnapshot& ds, std::map<const uint32_t*, SlotSet>& cache,
                                  const uint32_t* off, const uint32_t* nbr, uint32_t n_rows, const Derived* closure,
                                  uint32_t n_groups) {
  if (!e.delta_hint || !e.dev) return nullptr;
  const DeltaHint::Users* hu = nullptr;
  for (const DeltaHint::Users& u : e.delta_hint->users)
    if (u.t_off == off) hu = &u;
  if (!hu) return nullptr;
  const SlotRec* old = nullptr;
  for (const SlotRec& r : e.dev->slot_recs)
    if (r.kind == (uint8_t)SlotKind::kUser && r.src_off == hu->old_t_off && r.lab == closure->lab &&
        r.cov_pre == closure->cov_pre && r.n_rows == n_rows)
      old = &r;
  if (!old) return nullptr;
  PhaseClock pc("user_slots_delta");
  const uint32_t n = hu->n;
  uint32_t* staged = dalloc<uint32_t>(ds.allocs, (size_t)std::max<uint32_t>(n, 1) * kUSlotWords, &ds.bytes);
  std::vector<void*> tmp;
  uint32_t* list = nullptr;
  const uint64_t total = old->list_total;
  uint32_t add = 0;
  try {
    uint32_t* len = dalloc<uint32_t>(tmp, (size_t)n + 1);
    uint32_t* loff = dalloc<uint32_t>(tmp, (size_t)n + 1);
    HIP_OK(hipStreamSynchronize(nullptr));
    const uint32_t cap = ds.slot_bits == 24 ? (uint32_t)slot_cap<24>() : (uint32_t)slot_cap<32>();
    if (n) {
      hipLaunchKernelGGL(k_user_list_len_ids, dim3(grid_for(n)), dim3(kBlock), 0, 0, off, nbr, hu->ids, n, closure->lab,
                         closure->cov_off, n_groups, cap, len);
      HIP_OK(hipGetLastError());
    }
    device_excl_scan(len, n, loff);
    HIP_OK(hipMemcpy(&add, loff + n, 4, hipMemcpyDeviceToHost));
    if (total + add >= (1u << 31)) {  // (u32 list offsets: the full build decides)
      free_list(tmp);
      return nullptr;
    }
    if (add) {  // loff past the current lists
      hipLaunchKernelGGL(k_add_u32, dim3(grid_for(n)), dim3(kBlock), 0, 0, loff, n, (uint32_t)total);
      HIP_OK(hipGetLastError());
    }
    if (total + add > 0) {
      list = slot_alloc(ds, (size_t)(total + add) * 4);
      if (total) HIP_OK(hipMemcpy(list, old->list, total * 4, hipMemcpyDeviceToDevice));
    }
    if (n)
      launch_user_slots_ids(ds.slot_bits, off, nbr, hu->ids, n, closure->lab, closure->cov_off, closure->cov_pre, n_groups,
                            list ? loff : nullptr, list, staged);
    HIP_OK(hipDeviceSynchronize());
  } catch (...) {
    free_list(tmp);
    throw;
  }
  free_list(tmp);
  ds.adopt_h.push_back(old->slots);  // (the slot array passes to the new snapshot at publish)
  ds.slot_patches.push_back({old->slots, staged, hu->ids, n});
  ds.slot_recs.push_back({off, closure->lab, closure->cov_pre, old->slots, list, total + add, n_rows,
                          (uint8_t)SlotKind::kUser});
  SlotSet out;
  out.slots = old->slots;
  out.list = list;
  if (pc.on) pc.line += " users=" + std::to_string(n);
  return &(cache[off] = out);
}

static SlotSet slots_for(Engine& e, DeviceSnapshot& ds, std::map<const uint32_t*, SlotSet>& cache,
                         const uint32_t* off, const uint32_t* nbr, uint32_t n_rows, SlotKind kind,
                         const Derived* closure, uint32_t n_groups) {
  const uint32_t words = kind == SlotKind::kUser ? kUSlotWords : kDSlotWords;
  auto hit = cache.find(off);
  if (hit != cache.end()) return hit->second;
  // the current snapshot's slots over the same CSR and the same labels and covers: taken over at
  // publish as they are (a Watch batch that changed neither side)
  if (e.dev)
    for (const SlotRec& r : e.dev->slot_recs)
      if (r.kind == (uint8_t)kind && r.src_off == off && r.lab == closure->lab && r.cov_pre == closure->cov_pre &&
          r.n_rows == n_rows) {
        ds.adopt_h.push_back(r.slots);
        if (r.list) ds.adopt_h.push_back(r.list);
        ds.slot_recs.push_back(r);
        SlotSet out;
        out.slots = r.slots;
        out.list = r.list;
        return cache[off] = out;
      }
  if (kind == SlotKind::kUser)
    if (const SlotSet* d = slots_delta(e, ds, cache, off, nbr, n_rows, closure, n_groups)) return *d;
  PhaseClock pc(kind == SlotKind::kUser ? "user_slots" : "res_slots");
  const size_t bytes = (size_t)std::max<uint32_t>(n_rows, 1) * (words + (kind == SlotKind::kResource ? kFrontWords : 0u)) * 4;
  size_t free_b = 0, total_b = 0;
  HIP_OK(hipMemGetInfo(&free_b, &total_b));
  SlotSet out;
  if (bytes <= free_b / 2) {
    uint32_t* s = slot_alloc(ds, bytes);
    if (n_rows && kind == SlotKind::kUser) {
      // (the cover lists take at most half of the HBM that is free once the slots are allocated)
      const UserLists ul = build_user_slots(ds.slot_bits, off, nbr, n_rows, closure->lab, closure->cov_off, closure->cov_pre,
                                            n_groups, s, [&](size_t list_bytes) -> uint32_t* {
                                              size_t free2 = 0;
                                              HIP_OK(hipMemGetInfo(&free2, &total_b));
                                              return list_bytes <= free2 / 2 ? slot_alloc(ds, list_bytes) : nullptr;
                                            });
      ds.slot_recs.push_back({off, closure->lab, closure->cov_pre, s, ul.list, ul.list ? (uint64_t)ul.total : 0ull, n_rows,
                              (uint8_t)SlotKind::kUser});
      out.list = ul.list;
    } else if (n_rows) {
      hipLaunchKernelGGL(k_res_slots, dim3(grid_for(n_rows)), dim3(kBlock), 0, 0, off, nbr, n_rows, closure->lab,
                         n_groups, s, s + (size_t)n_rows * kDSlotWords);
      HIP_OK(hipGetLastError());
      HIP_OK(hipDeviceSynchronize());
      ds.slot_recs.push_back({off, closure->lab, closure->cov_pre, s, nullptr, 0ull, n_rows, (uint8_t)SlotKind::kResource});
    }
    out.slots = s;
  }
  cache[off] = out;
  return out;
}

// The closure-join stage's table (closure.inc): the eligible roots among the bidirectional ones.
static void build_closure_join(Engine& e, DeviceSnapshot& ds, const std::vector<DevNode>& nodes,
                               const std::vector<DevItem>& items, const std::vector<DevCSR>& table,
                               const std::vector<char>& elig, const std::vector<uint32_t>& jump,
                               const std::vector<uint32_t>& rec_csr, const std::unordered_map<uint32_t, uint32_t>& tmap) {
  ds.cj_host.clear();
  ds.cj_n_desc = 0;
  const uint32_t nf = ds.n_fwd;
  const uint32_t n_types = (uint32_t)e.schema->types.size();
  if (e.cfg.flags & GCK_FLAG_NO_CLOSURE) return;
  // m is a self-recursive relation with a closure whose items are the recursive userset kind and
  // plain direct subject kinds only
  auto m_ok = [&](uint32_t m) {
    if (m >= nf || jump[m] == kNone || nodes[m].kind != NK_RELATION) return false;
    const DevNode& nd = nodes[m];
    for (uint32_t k = 0; k < nd.count; ++k) {
      const DevItem& it = items[nd.first + k];
      if (it.kind != IT_KIND || it.csr_ext != kNone) return false;
      if (it.srel == kEllipsis) continue;
      if (!(it.srel == m && it.target == m && it.stype == nd.type && it.csr_plain == rec_csr[m])) return false;
    }
    return true;
  };
  const Derived* closure_of = nullptr;
  bool no_fronts = false;
  if (const char* f = debug_env("GCK_DEBUG_CJ_FRONT")) no_fronts = atoi(f) == 0;
  std::map<const uint32_t*, SlotSet> slot_cache;  // source CSR offsets -> its slots
  {
    ds.slot_bits = 24u;
    for (const Derived& x : ds.derived)
      if (x.kind == 1 && x.d.n_rows >= (1u << 24) - 1u) ds.slot_bits = 32;  // (all-ones: the unused-entry mark)
    // (GCK_DEBUG_SLOT_BITS=32: the 32-bit layout and its kernels on a small hierarchy, for the tests)
    if (const char* b = debug_env("GCK_DEBUG_SLOT_BITS"))
      if (atoi(b) == 32) ds.slot_bits = 32;
  }
  std::vector<uint16_t> root(nf, 0xFFFFu);
  std::vector<CjMeta> meta;
  std::vector<CjEntry> ents;
  for (uint32_t p = 0; p < nf && p < 0xFFFFu; ++p) {
    if (!elig[p]) continue;
    uint32_t n = p;
    for (int hop = 0; hop < 16 && nodes[n].kind == NK_UNION && nodes[n].count == 1 &&
                      items[nodes[n].first].kind == IT_COMPUTED && items[nodes[n].first].target < nf;
         ++hop)
      n = items[nodes[n].first].target;
    if (nodes[n].kind != NK_RELATION) continue;
    uint32_t m = kNone, vcsr = kNone;
    if (m_ok(n)) {
      m = n;  // V(R) = {R}
    } else if (nodes[n].count == 1) {
      const DevItem& it = items[nodes[n].first];
      if (it.kind == IT_KIND && it.srel != kEllipsis && it.csr_ext == kNone && it.csr_plain != kNone &&
          it.target == it.srel && m_ok(it.srel) && it.stype == nodes[it.srel].type) {
        m = it.srel;
        vcsr = it.csr_plain;
      }
    }
    if (m == kNone) continue;
    closure_of = nullptr;
    for (const Derived& x : ds.derived)
      if (x.kind == 1 && x.d.nbr == table[jump[m]].nbr) closure_of = &x;
    if (!closure_of || !closure_of->sig || !table[jump[m]].mhash) continue;
    CjMeta M{};
    M.mtype = nodes[m].type;
    M.mrel = (uint16_t)m;
    M.rtype = nodes[p].type;
    // the objects of m's type that the hierarchy's labels, covers and signatures cover: those the
    // closure was built over. A Watch batch that adds objects of the type without nesting them
    // keeps the closure; the new ones (no ancestors) are past its rows and stay off the slots
    // (their users' covers overflow to the task rounds, whose signature reads stop at m_rows)
    M.m_rows = std::min<uint32_t>(e.interner[nodes[m].type].count, closure_of->d.n_rows);
    for (uint32_t t = 0; t < n_types; ++t) {
      CjEntry E{};
      if (vcsr != kNone) {
        E.v_off = table[vcsr].off;
        E.v_nbr = table[vcsr].nbr;
        E.v_rows = table[vcsr].n_rows;
      }
      const DevNode& mn = nodes[m];
      for (uint32_t k = 0; k < mn.count; ++k) {
        const DevItem& it = items[mn.first + k];
        if (it.srel != kEllipsis || it.stype != t || it.csr_plain == kNone) continue;
        auto tr = tmap.find(it.csr_plain);
        if (tr == tmap.end()) continue;
        E.t_off = table[tr->second].off;
        E.t_nbr = table[tr->second].nbr;
        E.t_rows = table[tr->second].n_rows;
      }
      E.sig = closure_of->sig;
      E.anc_hash = table[jump[m]].mhash;
      E.anc_bmask = table[jump[m]].mmask;
      if (E.v_off && E.t_off && closure_of->lab && closure_of->cov_off && !(e.cfg.flags & GCK_FLAG_NO_SLOTS)) {
        const SlotSet us = slots_for(e, ds, slot_cache, E.t_off, E.t_nbr, E.t_rows, SlotKind::kUser, closure_of, M.m_rows);
        E.uslot = us.slots;
        E.ulist = us.list;
        const SlotSet rs = E.uslot ? slots_for(e, ds, slot_cache, E.v_off, E.v_nbr, E.v_rows, SlotKind::kResource, closure_of, M.m_rows)
                                   : SlotSet{};
        E.dslot = rs.slots;
        if (!E.dslot) E.uslot = E.ulist = nullptr;
        // the fronts' starts are 24 bits wide: 24-bit snapshots only (GCK_DEBUG_CJ_FRONT=0: the join without them)
        else if (ds.slot_bits == 24u && !no_fronts) E.dfront = rs.fronts(E.v_rows);
      }
      ents.push_back(E);
    }
    root[p] = (uint16_t)meta.size();
    meta.push_back(M);
  }
  if (meta.empty()) return;
  std::vector<unsigned char> blob;
  auto put = [&](const void* src, size_t bytes) {
    const size_t o = (blob.size() + 15) & ~(size_t)15;
    blob.resize(o + bytes);
    std::memcpy(blob.data() + o, src, bytes);
    return (uint32_t)o;
  };
  put(root.data(), root.size() * 2);
  const uint32_t o_meta = put(meta.data(), meta.size() * sizeof(CjMeta));
  const uint32_t o_ent = put(ents.data(), ents.size() * sizeof(CjEntry));
  blob.resize(cj_table_bytes(blob.size()));  // (the join stages it in 16-B chunks)
  if (blob.size() > kCjLdsBytes) return;  // too large to stage in LDS: the bundles take everything
  ds.cj_host = std::move(blob);
  ds.cj_n_desc = (uint32_t)meta.size();
  ds.cj_o_meta = o_meta;
  ds.cj_o_entries = o_ent;
}

// Builds the reverse program (see the top of this file) into `nodes` / `items` / `table`, and
// marks the eligible forward nodes NF_BIDIR. No-op when nothing is eligible.
static void build_bidir(Engine& e, DeviceSnapshot& ds, std::vector<DevNode>& nodes, std::vector<DevItem>& items,
                        std::vector<DevCSR>& table, const std::vector<CsrInfo>& info, std::vector<void*>& adopted) {
  const Schema& sc = *e.schema;
  const uint32_t nf = (uint32_t)nodes.size();
  const uint32_t n_types = (uint32_t)sc.types.size();
  ds.n_fwd = nf;
  if (e.cfg.flags & (GCK_FLAG_NO_BIDIR | GCK_FLAG_NO_MHASH)) return;
  if (2 * nf + n_types >= 4096) return;  // bundle visited keys hold 12-bit node ids
  const uint32_t max_depth = e.cfg.max_depth ? e.cfg.max_depth : 50;
  auto row_target = [&](const DevItem& it) -> uint32_t {  // the node a row edge enters, or kNone
    if (it.kind == IT_KIND) return it.srel == kEllipsis ? kNone : it.target;
    if (it.kind == IT_ARROW) return it.target == kNoNode ? kNone : it.target;
    return kNone;
  };
  // 1. nodes that are plain unions: stored relations, computed usersets, `->` arrows only
  std::vector<char> plain(nf, 1);
  for (uint32_t n = 0; n < nf; ++n) {
    const DevNode& nd = nodes[n];
    if (nd.kind != NK_RELATION && nd.kind != NK_UNION) plain[n] = 0;
    for (uint32_t k = 0; k < nd.count && plain[n]; ++k) {
      const DevItem& it = items[nd.first + k];
      if (it.kind == IT_SUB || it.kind == IT_OPERAND) plain[n] = 0;
      if (it.csr_ext != kNone) plain[n] = 0;  // caveated / expiring edges: CONDITIONAL semantics
      if (it.kind == IT_KIND && it.srel == kEllipsis && it.csr_plain != kNone) {
        const DevCSR& r = table[it.csr_plain];
        // wildcard rows, or not known (no index: GCK_FLAG_NO_MHASH; engine.hip scan_wild when too large)
        if (info[it.csr_plain].n_edges > 0 && ((!r.mhash && !(r.pad & kCsrWildKnown)) || r.has_wild)) plain[n] = 0;
      }
    }
  }
  // 2. closures (node graph) and the computed-only ("local") part of each
  auto succ = [&](uint32_t n, std::vector<std::pair<uint32_t, bool>>& out) {  // (target, is row edge)
    out.clear();
    const DevNode& nd = nodes[n];
    for (uint32_t k = 0; k < nd.count; ++k) {
      const DevItem& it = items[nd.first + k];
      if (it.kind == IT_COMPUTED) out.push_back({it.target, false});
      const uint32_t t = row_target(it);
      if (t != kNone && (it.csr_plain != kNone)) out.push_back({t, true});
    }
  };
  std::vector<std::vector<char>> clos(nf);
  std::vector<char> cand(nf, 0);
  std::vector<std::pair<uint32_t, bool>> nb;
  for (uint32_t p = 0; p < nf; ++p) {
    // state (node, remote): remote = reached through at least one row edge
    std::vector<char> seen(2 * nf, 0);
    std::vector<uint32_t> stack{p * 2};
    seen[p * 2] = 1;
    while (!stack.empty()) {
      const uint32_t s = stack.back();
      stack.pop_back();
      succ(s / 2, nb);
      for (auto [t, row] : nb) {
        const uint32_t ns = t * 2 + ((s & 1) | (row ? 1u : 0u));
        if (!seen[ns]) {
          seen[ns] = 1;
          stack.push_back(ns);
        }
      }
    }
    clos[p].assign(nf, 0);
    bool ok = true;
    uint32_t cm = 0, lm = 0;
    for (uint32_t t = 0; t < nf; ++t) {
      const bool local = seen[t * 2], remote = seen[t * 2 + 1];
      if (!(local || remote)) continue;
      clos[p][t] = 1;
      if (!plain[t]) ok = false;
      if (t < 32) {
        cm |= 1u << t;
        if (local && !remote) lm |= 1u << t;
      }
    }
    cand[p] = ok ? 1 : 0;
    nodes[p].cmask = cm;
    nodes[p].lmask = lm;
  }
  std::vector<char> used(nf, 0);  // nodes in some candidate closure
  bool any = false;
  for (uint32_t p = 0; p < nf; ++p)
    if (cand[p]) {
      any = true;
      for (uint32_t t = 0; t < nf; ++t) used[t] |= clos[p][t];
    }
  if (!any) return;
  // 3. heights: build_heights (heights.inc) relaxed them over every edge of the snapshot
  const std::vector<uint32_t>& hmax = ds.hmax;
  auto type_count = [&](uint32_t t) { return e.interner[t].count; };
  // 4. eligible roots: every forward path shorter than the depth budget
  std::vector<char> elig(nf, 0);
  std::fill(used.begin(), used.end(), 0);
  any = false;
  for (uint32_t p = 0; p < nf; ++p) {
    if (!cand[p] || hmax[p] >= max_depth) continue;
    elig[p] = 1;
    any = true;
    for (uint32_t t = 0; t < nf; ++t) used[t] |= clos[p][t];
  }
  if (!any) return;
  // 5. reverse program over the union of eligible closures, with transposed CSRs
  std::unordered_map<uint32_t, uint32_t> tmap;  // forward CSR -> transposed CSR (table index)
  auto transpose = [&](uint32_t c) -> uint32_t {
    auto f = tmap.find(c);
    if (f != tmap.end()) return f->second;
    const DevCSR r = table[c];
    const uint64_t ne = info[c].n_edges;
    if (const Derived* x = reuse_derived(e, 0, r, ne, adopted)) {
      ds.derived.push_back(*x);
      table.push_back(x->d);
      return tmap[c] = (uint32_t)table.size() - 1;
    }
    PhaseClock pc("transpose");
    const uint32_t n_sub = type_count(info[c].stype);
    uint32_t* off_t = dalloc<uint32_t>(ds.allocs, (size_t)n_sub + 1, &ds.bytes);
    uint32_t* nbr_t = dalloc<uint32_t>(ds.allocs, ne, &ds.bytes);
    std::vector<void*> t2;
    try {
      uint32_t* cnt = dalloc<uint32_t>(t2, n_sub);
      HIP_OK(hipMemset(cnt, 0, (size_t)std::max<uint32_t>(n_sub, 1) * 4));
      if (ne) hipLaunchKernelGGL(k_count_subjects, dim3(grid_for(ne)), dim3(kBlock), 0, 0, r.nbr,
                                 (unsigned long long)ne, n_sub, cnt);
      HIP_OK(hipGetLastError());
      device_excl_scan(cnt, n_sub, off_t);
      HIP_OK(hipMemcpy(cnt, off_t, (size_t)std::max<uint32_t>(n_sub, 1) * 4, hipMemcpyDeviceToDevice));
      if (ne) hipLaunchKernelGGL(k_transpose_scatter, dim3(grid_for(ne)), dim3(kBlock), 0, 0, r.off, r.nbr,
                                 r.n_rows, (unsigned long long)ne, n_sub, cnt, nbr_t);
      HIP_OK(hipGetLastError());
      HIP_OK(hipDeviceSynchronize());
    } catch (...) {
      free_list(t2);
      throw;
    }
    free_list(t2);
    DevCSR d{};
    d.off = off_t;
    d.nbr = nbr_t;
    d.n_rows = n_sub;
    table.push_back(d);
    ds.derived.push_back({0, r.nbr, ne, d});
    const uint32_t idx = (uint32_t)table.size() - 1;
    tmap[c] = idx;
    return idx;
  };
  // a node local to some eligible root: its reverse in-edges are probed on the forward CSR
  std::vector<char> local_any(nf, 0);
  for (uint32_t p = 0; p < nf; ++p)
    if (elig[p])
      for (uint32_t t = 0; t < nf && t < 32; ++t)
        if ((nodes[p].lmask >> t) & 1u) local_any[t] = 1;
  // 6. self-recursive usersets (`relation member: ... | group#member` on group): the ancestor
  //    closure of each object replaces the level-by-level reverse climb with one jump
  std::vector<uint32_t> rec_csr(nf, kNone), jump(nf, kNone);
  for (uint32_t n = 0; n < nf; ++n) {
    if (!used[n]) continue;
    const DevNode& nd = nodes[n];
    for (uint32_t k = 0; k < nd.count; ++k) {
      const DevItem& it = items[nd.first + k];
      if (it.kind == IT_KIND && it.srel != kEllipsis && it.target == n && it.stype == nd.type &&
          it.csr_plain != kNone && info[it.csr_plain].n_edges)
        rec_csr[n] = it.csr_plain;
    }
    if (rec_csr[n] != kNone)
      jump[n] = build_ancestors(e, ds, table, table[rec_csr[n]], info[rec_csr[n]].n_edges, adopted);
  }
  // 7. in-edges per reverse slot: [0, nf) rev(t); [nf, nf + types) S(type)
  struct InEdge {
    uint8_t kind;
    uint32_t fwd_csr;  // IT_REV: the forward CSR (kNone for the ancestor jump)
    uint32_t csr;      // IT_REV: the CSR enumerated (transpose or ancestor closure)
    uint32_t src;      // the node entered: rev(src) / rev'(src)
    bool to_partial;   // enters rev'(src) (ancestor jump)
    bool recursive;    // the self-recursive in-edge (replaced by the jump)
  };
  std::vector<std::vector<InEdge>> in(nf + n_types);
  for (uint32_t n = 0; n < nf; ++n) {
    if (!used[n]) continue;
    const DevNode& nd = nodes[n];
    for (uint32_t k = 0; k < nd.count; ++k) {
      const DevItem it = items[nd.first + k];
      if (it.kind == IT_COMPUTED) {
        in[it.target].push_back({IT_COMPUTED, kNone, kNone, n, false, false});
      } else if (it.kind == IT_KIND && it.csr_plain != kNone) {
        const uint32_t slot = it.srel == kEllipsis ? nf + it.stype : it.target;
        in[slot].push_back({IT_REV, it.csr_plain, transpose(it.csr_plain), n, false, it.csr_plain == rec_csr[n]});
      } else if (it.kind == IT_ARROW && it.target != kNoNode && it.csr_plain != kNone) {
        in[it.target].push_back({IT_REV, it.csr_plain, transpose(it.csr_plain), n, false, false});
      }
    }
  }
  // 8. emit the reverse nodes: rev(t) = nf + t, S(type) = 2 nf + type, then rev'(t) for every
  //    t with an ancestor closure (rev(t) without the recursive in-edge, entered by the jump).
  //    `canon` maps rev'(t) onto rev(t) (one visited key); a reverse node's `cmask` lists the
  //    forward nodes its probe-capable in-edges enter (bit 31: it has another kind of item)
  std::vector<uint32_t> partial_id(nf, kNone);
  uint32_t next_id = 2 * nf + n_types;
  for (uint32_t t = 0; t < nf; ++t)
    if (jump[t] != kNone) partial_id[t] = next_id++;
  if (next_id >= 4096) throw Error(GCK_E_SCHEMA, "schema too large for the bidirectional program");
  auto emit = [&](uint16_t type, uint32_t canon, const std::vector<InEdge>& es, bool partial, uint32_t jump_from) {
    DevNode rn{};
    rn.type = type;
    rn.kind = NK_UNION;
    rn.canon = (uint16_t)canon;
    rn.first = (uint32_t)items.size();
    uint32_t cm = 0;
    auto push_item = [&](uint8_t kind, uint32_t csr, uint32_t fwd_csr, uint32_t target_node, uint32_t src) {
      DevItem it{};
      it.kind = kind;
      it.stype = nodes[src].type;
      it.srel = kEllipsis;
      it.target = (uint16_t)target_node;
      it.csr_plain = csr;
      it.csr_ext = fwd_csr;
      for (uint32_t k = rn.first; k < items.size(); ++k)
        if (items[k].kind == kind && items[k].csr_plain == csr && items[k].target == it.target) return;
      items.push_back(it);
      const bool probe = kind == IT_REV && fwd_csr != kNone && src < 31 && local_any[src] && table[fwd_csr].mhash;
      cm |= probe ? (1u << src) : (1u << 31);
    };
    if (jump_from != kNone && !partial) {
      push_item(IT_REV, jump[jump_from], kNone, partial_id[jump_from], jump_from);
      rn.flags |= NF_JUMP;
    }
    for (const InEdge& x : es) {
      if (x.recursive && jump_from != kNone) continue;  // covered by the jump
      const uint32_t tgt = nf + x.src;
      if (x.kind == IT_REV && local_any[x.src] && !table[x.fwd_csr].mhash && info[x.fwd_csr].n_edges &&
          mhash_affordable(e, info[x.fwd_csr].n_edges))
        build_mhash(ds, table[x.fwd_csr], info[x.fwd_csr].n_edges);  // for the local probe (not above 4 GB)
      push_item(x.kind, x.csr, x.kind == IT_REV ? x.fwd_csr : kNone, tgt, x.src);
    }
    rn.count = (uint32_t)items.size() - rn.first;
    rn.cmask = cm;
    nodes.push_back(rn);
  };
  for (uint32_t t = 0; t < nf; ++t) emit(nodes[t].type, nf + t, in[t], false, jump[t] != kNone ? t : kNone);
  for (uint32_t ty = 0; ty < n_types; ++ty) emit((uint16_t)ty, 2 * nf + ty, in[nf + ty], false, kNone);
  for (uint32_t t = 0; t < nf; ++t)
    if (jump[t] != kNone) emit(nodes[t].type, nf + t, in[t], true, t);
  build_closure_join(e, ds, nodes, items, table, elig, jump, rec_csr, tmap);
  // the row each check of root p caches (in LDS): the forward CSR probed by the single item of a
  // probe-only reverse node that the ancestor jump enters (nested groups listed on a resource)
  for (uint32_t p = 0; p < nf; ++p) {
    nodes[p].canon = (uint16_t)p;
    nodes[p].lcsr = 0xFFFFu;
    if (!elig[p]) continue;
    nodes[p].flags |= NF_BIDIR;
    for (uint32_t t = 0; t < nf && nodes[p].lcsr == 0xFFFFu; ++t) {
      if (partial_id[t] == kNone) continue;
      const DevNode& rn = nodes[partial_id[t]];
      if (rn.count != 1 || (rn.cmask & ~(nodes[p].lmask & 0x7FFFFFFFu))) continue;
      const DevItem& li = items[rn.first];
      if (li.csr_ext < 0xFFFFu) nodes[p].lcsr = (uint16_t)li.csr_ext;
    }
  }
  ds.has_bidir = true;
}
