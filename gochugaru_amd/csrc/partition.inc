// partition.inc — graphs partitioned by object id over ranks (included by engine.hip).
//
// SURVEY.md §8e / BASELINE.json config 4, partitioned mode: a graph above one GPU's HBM is split
// over W ranks, one process per GPU. Rank r owns the objects with part_owner(obj) == r
// (gck_internal.hpp: id mod W) and holds (engine.hpp part_keep, applied at every ingest path):
//
//   * the rows of the objects it owns, complete — what the level loop expands — except of the
//     hub relations (group#member), whose tuples are kept by subject:
//   * the schema's hub hierarchy (labels_build.inc partition_rules: the userset / wildcard tuples of
//     the hub relations, group#member@group#member), replicated — the hierarchy labels;
//   * the hub tuples of the subjects it owns (group#member@user:u, owner(u) = r) — their user
//     slots, at part_local(u). A group's direct members live with the members' owners, not with
//     the group's: the level loop expands a hub's nodes at the owner of the check's subject
//     (part_dest), which holds everything such an entry reads, and no rank holds (or interns)
//     the members of the groups it owns.
//
// Nothing else of another rank's rows reaches it: a caller's device CSR is filtered while it is
// copied (part_filter_device), staged tuples and Watch updates as they arrive.
//
// A batch (every rank the same items, gck_part_check / gck_part_check_with):
//
//   1. the label join (labels.inc k_pj_*): the owner of a check's subject sends (check, user slot)
//      to the owner of its resource, which decides it from its resource slot; an all-reduce MAX of
//      the result bytes gives every rank every decided check;
//   2. the level loop over what no rank decided, in batch order on every rank, exact-depth (no
//      rank has the global heights) with joins: per level
//        expand   k_expand / k_edges over this rank's frontier; pushes for objects another rank
//                 owns go to its outbox (push_entry); intersection / exclusion / all() / caveat
//                 and-queries allocate query and join ids from this rank's own range (Ctx q_hi,
//                 j_hi), so ids are global without coordination
//        exchange one all-to-all: per peer a header (entries, new query / join ids), then the
//                 entries owed to it and the query / join records created this level (the same
//                 to every peer): every rank then holds every query and join of the batch
//        ingest   received entries pushed at the owner (visited dedupe), imported joins counted
//                 into their parent's pending joins
//        flags    found-Y / found-C / depth-error / alive planes over every allocated query, OR-ed
//                 by an all-reduce MAX, so every rank resolves every query identically (k_resolve:
//                 joins, cancellation, the tri-state algebra) and knows when the batch is done.
//
// The exchange runs over a transport (gck.h gck_transport): RCCL inside libgck (gck_part_check;
// grouped ncclSend / ncclRecv and ncclAllReduce over xGMI), or the caller's (gck_part_check_with;
// the tests drive it over gloo with ranks sharing one GPU).

// ---- ingest: a caller's device CSR, filtered while it is copied --------------------------------

__device__ __forceinline__ bool pkeep(uint32_t row, uint32_t x, uint32_t rank, uint32_t world, uint32_t hub,
                                      uint32_t userset) {
  if (!hub) return part_owner(row, world) == rank;
  return userset || x == kWildcard || part_owner(x, world) == rank;  // (engine.hpp part_keep)
}

// Per block of 256 edges: the kept edges as four 64-bit masks, and their count.
__global__ void __launch_bounds__(kBlock) k_pkeep_mark(const uint32_t* __restrict__ off, const uint32_t* __restrict__ nbr,
                                                       uint32_t n_rows, unsigned long long n_edges, uint32_t rank,
                                                       uint32_t world, uint32_t hub, uint32_t userset,
                                                       unsigned long long* __restrict__ bits, uint32_t* __restrict__ bcnt) {
  __shared__ uint32_t rows[2];
  __shared__ uint32_t s_cnt[kWaves];
  const unsigned long long e0 = (unsigned long long)blockIdx.x * kBlock;
  const unsigned long long e = e0 + threadIdx.x;
  const uint32_t o = block_edge_row(off, n_rows, n_edges, e0, e < n_edges ? e : n_edges - 1, rows);
  const bool keep = e < n_edges && pkeep(o, nbr[e], rank, world, hub, userset);
  const unsigned long long m = __ballot(keep);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    bits[(size_t)blockIdx.x * kWaves + wv] = m;
    s_cnt[wv] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < kWaves; ++w) t += s_cnt[w];
    bcnt[blockIdx.x] = t;
  }
}

// Kept edges below edge position `e` (bpos: exclusive scan of the block counts).
__device__ __forceinline__ uint32_t pkeep_rank(const unsigned long long* bits, const uint32_t* bpos, uint32_t n_blocks,
                                               unsigned long long e) {
  const unsigned long long b = e / kBlock;
  if (b >= n_blocks) return bpos[n_blocks];
  uint32_t at = bpos[b];
  const uint32_t in = (uint32_t)(e - b * kBlock);
  for (uint32_t w = 0; w < in / 64; ++w) at += (uint32_t)__popcll(bits[b * kWaves + w]);
  if (in & 63) at += (uint32_t)__popcll(bits[b * kWaves + in / 64] & ((1ull << (in & 63)) - 1ull));
  return at;
}

__global__ void __launch_bounds__(kBlock) k_pkeep_place(const uint32_t* __restrict__ nbr, unsigned long long n_edges,
                                                        const unsigned long long* __restrict__ bits,
                                                        const uint32_t* __restrict__ bpos, uint32_t n_blocks,
                                                        uint32_t* __restrict__ nnbr) {
  const unsigned long long e = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_edges) return;
  if (!((bits[e / 64] >> (e & 63)) & 1ull)) return;
  nnbr[pkeep_rank(bits, bpos, n_blocks, e)] = nbr[e];
}

__global__ void __launch_bounds__(kBlock) k_pkeep_off(const uint32_t* __restrict__ off, uint32_t n_rows,
                                                      const unsigned long long* __restrict__ bits,
                                                      const uint32_t* __restrict__ bpos, uint32_t n_blocks,
                                                      uint32_t* __restrict__ noff) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r > n_rows) return;
  noff[r] = pkeep_rank(bits, bpos, n_blocks, off[r]);
}

// A device CSR the caller loaded (gck_load_csr GCK_MEM_DEVICE), copied into the snapshot with only
// the edges this rank keeps (engine.hpp part_keep): the rows stay in order, so the copy is a
// sorted CSR again. Never more than the kept edges of it are allocated for the snapshot.
static void part_filter_device(const Engine& e, DeviceSnapshot& ds, const HostCSR& h, DevCSR& d, uint64_t& ne) {
  const uint32_t n = h.n_rows;
  const bool hub = h.rel < e.part_hub_rel.size() && e.part_hub_rel[h.rel];
  const uint32_t n_blocks = (uint32_t)((ne + kBlock - 1) / kBlock);
  std::vector<void*> tmp;
  try {
    unsigned long long* bits = dalloc<unsigned long long>(tmp, (size_t)std::max<uint32_t>(n_blocks, 1) * kWaves);
    uint32_t* bcnt = dalloc<uint32_t>(tmp, std::max<uint32_t>(n_blocks, 1));
    uint32_t* bpos = dalloc<uint32_t>(tmp, (size_t)n_blocks + 1);
    if (n_blocks) {
      hipLaunchKernelGGL(k_pkeep_mark, dim3(n_blocks), dim3(kBlock), 0, 0, h.dev_off, h.dev_nbr, n,
                         (unsigned long long)ne, e.part_rank, e.part_world, hub ? 1u : 0u,
                         h.srel != kEllipsis ? 1u : 0u, bits, bcnt);
      HIP_OK(hipGetLastError());
    }
    device_excl_scan(bcnt, n_blocks, bpos);
    uint32_t kept = 0;
    HIP_OK(hipMemcpy(&kept, bpos + n_blocks, 4, hipMemcpyDeviceToHost));
    uint32_t* noff = dalloc<uint32_t>(ds.allocs, (size_t)n + 1, &ds.bytes);
    uint32_t* nnbr = dalloc<uint32_t>(ds.allocs, kept, &ds.bytes);
    if (n_blocks)
      hipLaunchKernelGGL(k_pkeep_place, dim3(n_blocks), dim3(kBlock), 0, 0, h.dev_nbr, (unsigned long long)ne, bits, bpos,
                         n_blocks, nnbr);
    hipLaunchKernelGGL(k_pkeep_off, dim3(grid_for((uint64_t)n + 1)), dim3(kBlock), 0, 0, h.dev_off, n, bits, bpos,
                       n_blocks, noff);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    d.off = noff;
    d.nbr = nnbr;
    ne = kept;
  } catch (...) {
    free_list(tmp);
    throw;
  }
  free_list(tmp);
}

// ---- level-loop kernels -------------------------------------------------------------------------

// Roots of the batch (k_init wrote one per check into `roots`): the owner of a check's resource
// starts it; every rank keeps every check's query state.
__global__ void __launch_bounds__(kBlock) k_part_roots(Ctx c, const Entry* __restrict__ roots, uint32_t n,
                                                       Entry* __restrict__ fr0) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const Entry e = roots[i];
  if (qflags(&c.queries[i]) & QF_DONE) return;
  if (part_dest(c, e.q, e.obj, e.node) != c.rank) return;
  const unsigned idx = atomicAdd(&c.ctr->next_size, 1u);
  fr0[idx] = e;
}

// Received entries: pushed into the next frontier with the owner's visited dedupe.
__global__ void __launch_bounds__(kBlock) k_part_ingest(Ctx c, const Entry* __restrict__ in, uint32_t n) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const Entry e = in[i];
  if (e.q >= c.query_cap || part_dest(c, e.q, e.obj, e.node) != c.rank) {
    atomicOr(&c.ctr->overflow, 64u);  // malformed exchange
    return;
  }
  if (qflags(&c.queries[e.q]) & QF_DONE) return;
  push_entry(c, e.q, e.obj, e.node, e.depth, e.cond);
}

// Joins another rank created (their records already copied in): each holds one pending join of its
// parent query, as spawn_join / spawn_and counted it on the creating rank.
__global__ void __launch_bounds__(kBlock) k_part_adopt_joins(DevQuery* __restrict__ queries, const DevJoin* __restrict__ joins,
                                                             uint32_t n, uint32_t query_cap, DevCounters* ctr) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = joins[i].parent_q;
  if (p >= query_cap) {
    atomicOr(&ctr->overflow, 64u);
    return;
  }
  __hip_atomic_fetch_add(&queries[p].pending_joins, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The allocated query ids of a batch: [0, n) and each rank's range, concatenated into the flag
// planes' index space.
constexpr int kPartMaxRanges = 64;
struct PartRanges {
  uint32_t n;
  uint32_t lo[kPartMaxRanges], at[kPartMaxRanges + 1];
};

__device__ __forceinline__ uint32_t part_qid(const PartRanges& R, uint32_t m) {
  uint32_t k = 0;
  while (k + 1 < R.n && R.at[k + 1] <= m) ++k;
  return R.lo[k] + (m - R.at[k]);
}

// Flag planes of the M allocated queries (u8, 0/1): [0,M) found Y, [M,2M) found C, [2M,3M) depth
// error, [3M,4M) alive at the next level; byte 4M: this rank overflowed a buffer.
__global__ void __launch_bounds__(kBlock) k_part_export(Ctx c, PartRanges R, uint32_t M, uint8_t* __restrict__ fl) {
  const uint32_t m = blockIdx.x * kBlock + threadIdx.x;
  if (m == 0) fl[4 * (size_t)M] = c.ctr->overflow ? 1u : 0u;
  if (m >= M) return;
  const uint32_t q = part_qid(R, m);
  const uint32_t f = qflags(&c.queries[q]);
  fl[m] = (f & QF_FOUND_Y) ? 1u : 0u;
  fl[M + m] = (f & QF_FOUND_C) ? 1u : 0u;
  fl[2 * (size_t)M + m] = (f & QF_ERR) ? 1u : 0u;
  fl[3 * (size_t)M + m] = c.queries[q].last_alive > c.level ? 1u : 0u;
}

__global__ void __launch_bounds__(kBlock) k_part_import(Ctx c, PartRanges R, uint32_t M, const uint8_t* __restrict__ fl) {
  const uint32_t m = blockIdx.x * kBlock + threadIdx.x;
  if (m >= M) return;
  const uint32_t q = part_qid(R, m);
  uint32_t bits = 0;
  if (fl[m]) bits |= QF_FOUND_Y;
  if (fl[M + m]) bits |= QF_FOUND_C;
  if (fl[2 * (size_t)M + m]) bits |= QF_ERR;
  if (bits) atomicOr(&c.queries[q].flags, bits);
  if (fl[3 * (size_t)M + m]) c.queries[q].last_alive = c.level + 1;
}

// k_resolve over the query ids [lo, hi) (one range of the batch).
__global__ void __launch_bounds__(kBlock) k_resolve_range(Ctx c, uint32_t lo, uint32_t hi) {
  if (__hip_atomic_load(&c.ctr->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t qi = lo + blockIdx.x * blockDim.x + threadIdx.x; qi < hi; qi += stride) resolve_query(c, qi);
}

__global__ void __launch_bounds__(kBlock) k_iota(uint32_t* __restrict__ idx, uint32_t n) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) idx[i] = i;
}

// Checks still undecided (identical on every rank after the resolve).
__global__ void __launch_bounds__(kBlock) k_part_open(Ctx c, uint32_t n, unsigned* open) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool o = i < n && !(qflags(&c.queries[i]) & QF_DONE);
  const unsigned long long m = __ballot(o);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(open, (unsigned)__popcll(m));
}

// ---- host side ----------------------------------------------------------------------------------

static void part_require(Engine& e) {
  if (e.part_world < 1) throw Error(GCK_E_STATE, "engine partition not set (gck_set_partition)");
}

// The transport of a batch: the caller's (gck_part_check_with) or RCCL's; failures are errors.
struct Xport {
  const gck_transport* t;
  uint32_t rank, world;
  void alltoallv(const void* send, const std::vector<uint64_t>& sb, void* recv, const std::vector<uint64_t>& rb,
                 hipStream_t st) const {
    if (world <= 1) return;
    if (t->alltoallv(t->ctx, send, sb.data(), recv, rb.data(), st) != 0)
      throw Error(GCK_E_DEVICE, "partition transport: all-to-all failed");
  }
  void allreduce_max(void* buf, uint64_t n, hipStream_t st) const {
    if (world <= 1 || n == 0) return;
    if (t->allreduce_max_u8(t->ctx, buf, n, st) != 0) throw Error(GCK_E_DEVICE, "partition transport: all-reduce failed");
  }
};

// A device byte buffer that grows (contents not kept).
struct PartBuf {
  uint8_t* p = nullptr;
  size_t cap = 0;
  uint8_t* want(size_t bytes) {
    if (cap < bytes) {
      if (p) HIP_OK(hipFree(p));
      p = nullptr;
      cap = std::max(bytes, 2 * cap);
      HIP_OK(hipMalloc(&p, cap));
    }
    return p;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct PartState {
  uint32_t world = 0;
  // the label join: per destination rank a region of `cap` records
  size_t cap = 0;
  uint32_t* out = nullptr;
  unsigned* cnt = nullptr;       // [world] records per destination, [world] overflow
  unsigned* h_cnt = nullptr;     // pinned mirror (also the leftover count)
  uint32_t* flag = nullptr;      // leftover compaction: block counts, positions, indices, items, results
  uint32_t* pos = nullptr;
  uint32_t* idx = nullptr;
  gck_item* left = nullptr;
  uint8_t* lperm = nullptr;
  int32_t* lerr = nullptr;
  // the level loop
  Entry* outbox = nullptr;       // world regions of out_cap entries
  unsigned* out_cnt = nullptr;   // [world] entries per destination, [world] open checks
  uint32_t out_cap = 0;
  unsigned* h_out = nullptr;     // pinned: out_cnt mirror
  DevCounters* h_ctr = nullptr;  // pinned: the counters after an expand
  uint64_t* h_hdr = nullptr;     // pinned: headers sent [world * 5], received [world * 5]
  PartBuf hdr, send, recv, flags, misc, sub;
};  // (created, grown and used under the partition workspace's mutex, part_run)

static PartState& part_state(Workspace& w);  // engine.hip

static void free_part(PartState* p) {
  if (!p) return;
  for (void* q : {(void*)p->out, (void*)p->cnt, (void*)p->flag, (void*)p->pos, (void*)p->idx, (void*)p->left,
                  (void*)p->lperm, (void*)p->lerr})
    if (q) (void)hipFree(q);
  for (void* q : {(void*)p->h_cnt, (void*)p->h_out, (void*)p->h_ctr, (void*)p->h_hdr})
    if (q) (void)hipHostFree(q);
  for (PartBuf* b : {&p->hdr, &p->send, &p->recv, &p->flags, &p->misc, &p->sub}) b->release();
  delete p;  // outbox / out_cnt are in the workspace's allocation list
}

// The buffers of a batch of n checks on `world` ranks (grown, never shrunk).
static PartState& part_bufs(Engine& e, Workspace& w, size_t n) {
  PartState& p = part_state(w);
  const uint32_t world = e.part_world;
  if (p.world != world || p.cap < n) {
    for (void* q : {(void*)p.out, (void*)p.cnt, (void*)p.flag, (void*)p.pos, (void*)p.idx, (void*)p.left,
                    (void*)p.lperm, (void*)p.lerr})
      if (q) HIP_OK(hipFree(q));
    p.cap = std::max<size_t>(n, 1024);
    HIP_OK(hipMalloc(&p.out, p.cap * world * kPjRecWords * 4));
    HIP_OK(hipMalloc(&p.cnt, (world + 1) * 4));
    HIP_OK(hipMalloc(&p.flag, p.cap * 4));
    HIP_OK(hipMalloc(&p.pos, (p.cap + 1) * 4));
    HIP_OK(hipMalloc(&p.idx, p.cap * 4));
    HIP_OK(hipMalloc(&p.left, p.cap * sizeof(gck_item)));
    HIP_OK(hipMalloc(&p.lperm, p.cap));
    HIP_OK(hipMalloc(&p.lerr, p.cap * 4));
  }
  if (p.world != world) {
    if (world + 1 > kPartMaxRanges) throw Error(GCK_E_CAPACITY, "at most 63 ranks");
    p.world = world;
    p.out_cap = (uint32_t)std::max<size_t>(w.frontier_cap / world, 1024);
    p.outbox = dalloc<Entry>(w.allocs, (size_t)p.out_cap * world);
    p.out_cnt = dalloc<unsigned>(w.allocs, world + 1);
    HIP_OK(hipStreamSynchronize(nullptr));  // pool allocations are ordered on the null stream
    for (void* q : {(void*)p.h_cnt, (void*)p.h_out, (void*)p.h_ctr, (void*)p.h_hdr})
      if (q) HIP_OK(hipHostFree(q));
    HIP_OK(hipHostMalloc(&p.h_cnt, (kPartMaxRanges + 1) * 4, hipHostMallocDefault));
    HIP_OK(hipHostMalloc(&p.h_out, (kPartMaxRanges + 1) * 4, hipHostMallocDefault));
    HIP_OK(hipHostMalloc(&p.h_ctr, sizeof(DevCounters), hipHostMallocDefault));
    HIP_OK(hipHostMalloc(&p.h_hdr, 2 * kPartMaxRanges * 5 * 8, hipHostMallocDefault));
  }
  return p;
}

static LjTab lj_tab(const DeviceSnapshot& ds) { return LjTab{ds.d_lj, ds.n_fwd, ds.lj.o_meta}; }

static void add_join_stats(Engine& e, size_t n, size_t n_left) {
  std::lock_guard<std::mutex> sl(e.stats_mu);
  e.stats.closure_checks += n - n_left;
  e.stats.slot_checks += n - n_left;
  e.stats.label_checks += n - n_left;
}

static constexpr size_t kHdrWords = 5;  // per peer: entries, first query id, queries, first join id, joins
static size_t pad8(size_t b) { return (b + 7) & ~(size_t)7; }

// The level loop over n checks (every rank the same items): false when a rank overflowed a buffer
// or its id range (every rank sees it in the reduced flags; the caller retries with fewer checks).
static bool part_loop(Engine& e, const Xport& X, Workspace& w, PartState& p, const gck_item* d_items, uint32_t n,
                      int64_t now_us, uint8_t* d_perm, int32_t* d_err, hipStream_t st) {
  const uint32_t W = e.part_world, r = e.part_rank;
  Ctx c = make_ctx(e, w, now_us, st);
  c.ck_items = d_items;
  c.rank = r;
  c.world = W;
  c.outbox = p.outbox;
  c.out_cnt = p.out_cnt;
  c.out_cap = p.out_cap;
  c.n_ctx = 0;  // (check-time caveat contexts are not taken in this mode)
  c.force_exact = W > 1 ? 1u : 0u;  // no rank has the global heights: every check exact-depth
  c.part_sub = nullptr;
  if (W > 1) {  // the hubs' nodes: expanded at the owner of the check's subject (part_dest)
    const DeviceSnapshot& ds = *e.dev;
    std::vector<uint8_t> f(std::max<uint32_t>(ds.n_nodes, 1), 0);
    for (size_t k = 0; k < e.part_sub_node.size() && k < f.size(); ++k) f[k] = e.part_sub_node[k];
    uint8_t* d = p.sub.want(f.size());
    HIP_OK(hipMemcpyAsync(d, f.data(), f.size(), hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));  // (f is pageable and dies with this scope)
    c.part_sub = d;
  }
  if (c.query_cap <= n || c.join_cap < W) return false;
  const uint32_t QR = (c.query_cap - n) / W, JR = c.join_cap / W;
  if (QR == 0) return false;
  std::vector<uint32_t> q_base(W), q_end(W), j_base(W), j_end(W);
  for (uint32_t s = 0; s < W; ++s) {
    q_base[s] = q_end[s] = n + s * QR;
    j_base[s] = j_end[s] = s * JR;
  }
  c.q_hi = q_base[r] + QR;
  c.j_hi = j_base[r] + JR;
  HIP_OK(hipMemsetAsync(w.ctr, 0, sizeof(DevCounters), st));
  HIP_OK(hipMemsetAsync(w.visited, 0xFF, w.visited_cap * sizeof(unsigned long long), st));
  DevCounters* init = p.h_ctr;
  *init = DevCounters{};
  init->n_queries = q_base[r];
  init->n_joins = j_base[r];
  HIP_OK(hipMemcpyAsync(w.ctr, init, sizeof(DevCounters), hipMemcpyHostToDevice, st));
  w.ctr_clean = false;
  c.level = 0;
  hipLaunchKernelGGL(k_init, dim3(grid_for(n)), dim3(kBlock), 0, st, c, d_items, n, w.fr[1], w.item_err);
  hipLaunchKernelGGL(k_part_roots, dim3(grid_for(n)), dim3(kBlock), 0, st, c, w.fr[1], n, w.fr[0]);
  hipLaunchKernelGGL(k_level_end, dim3(1), dim3(1), 0, st, w.ctr);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(p.h_ctr, w.ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  uint32_t n_cur = p.h_ctr->last_next, cur = 0;
  const uint32_t level_cap = 64 * c.max_depth + 64;
  std::vector<uint64_t> sb(W), rb(W);
  uint64_t levels = 0;
  for (uint32_t level = 0;; ++level) {
    if (level > level_cap) throw Error(GCK_E_DEVICE, "level cap exceeded (engine invariant)");
    c.level = level;
    c.next = w.fr[cur ^ 1];
    // 1. expand this rank's frontier
    HIP_OK(hipMemsetAsync(p.out_cnt, 0, (W + 1) * sizeof(unsigned), st));
    if (n_cur) {
      hipLaunchKernelGGL(k_expand, dim3(grid_for(n_cur)), dim3(kBlock), 0, st, c, w.fr[cur], n_cur);
      hipLaunchKernelGGL(k_edges, dim3(2048), dim3(kBlock), 0, st, c);
      HIP_OK(hipGetLastError());
    }
    HIP_OK(hipMemcpyAsync(p.h_out, p.out_cnt, W * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(p.h_ctr, w.ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const uint32_t my_q = std::min<uint32_t>(p.h_ctr->n_queries, c.q_hi);
    const uint32_t my_j = std::min<uint32_t>(p.h_ctr->n_joins, c.j_hi);
    const uint32_t nq = my_q - q_end[r], nj = my_j - j_end[r];
    // 2. exchange: headers, then per peer [entries owed to it][new queries][new joins]
    std::vector<uint64_t> hs(W * kHdrWords, 0), rh(W * kHdrWords, 0);  // per rank (self: zeros)
    if (W > 1) {
      for (uint32_t d = 0; d < W; ++d) {
        if (d == r) continue;
        uint64_t* h = &hs[d * kHdrWords];
        h[0] = std::min<uint32_t>(p.h_out[d], p.out_cap);
        h[1] = q_end[r], h[2] = nq, h[3] = j_end[r], h[4] = nj;
      }
      // (the packed send holds the peers' blocks in rank order, self skipped)
      for (uint32_t d = 0, k = 0; d < W; ++d) {
        sb[d] = rb[d] = d == r ? 0 : kHdrWords * 8;
        if (d != r) std::copy(&hs[d * kHdrWords], &hs[(d + 1) * kHdrWords], p.h_hdr + (k++) * kHdrWords);
      }
      uint8_t* dh = p.hdr.want(2 * W * kHdrWords * 8);
      HIP_OK(hipMemcpyAsync(dh, p.h_hdr, (W - 1) * kHdrWords * 8, hipMemcpyHostToDevice, st));
      X.alltoallv(dh, sb, dh + W * kHdrWords * 8, rb, st);
      HIP_OK(hipMemcpyAsync(p.h_hdr + W * kHdrWords, dh + W * kHdrWords * 8, (W - 1) * kHdrWords * 8,
                            hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      for (uint32_t s = 0, k = 0; s < W; ++s)
        if (s != r) {
          const uint64_t* src = p.h_hdr + W * kHdrWords + (k++) * kHdrWords;
          std::copy(src, src + kHdrWords, rh.begin() + s * kHdrWords);
        }
      // the data: sizes, send buffer
      const size_t q_bytes = (size_t)nq * sizeof(DevQuery), j_bytes = (size_t)nj * sizeof(DevJoin);
      size_t s_total = 0, r_total = 0;
      for (uint32_t d = 0; d < W; ++d) {
        if (d == r) {
          sb[d] = rb[d] = 0;
          continue;
        }
        sb[d] = pad8(hs[d * kHdrWords] * sizeof(Entry)) + q_bytes + j_bytes;
        const uint64_t* h = &rh[d * kHdrWords];
        if (h[1] != q_end[d] || h[3] != j_end[d] || h[1] + h[2] > q_base[d] + QR || h[3] + h[4] > j_base[d] + JR)
          throw Error(GCK_E_DEVICE, "partitioned check: peer id ranges disagree (engine invariant)");
        rb[d] = pad8(h[0] * sizeof(Entry)) + h[2] * sizeof(DevQuery) + h[4] * sizeof(DevJoin);
        s_total += sb[d];
        r_total += rb[d];
      }
      uint8_t* sendp = p.send.want(std::max<size_t>(s_total, 8));
      uint8_t* recvp = p.recv.want(std::max<size_t>(r_total, 8));
      size_t at = 0;
      for (uint32_t d = 0; d < W; ++d) {
        if (d == r) continue;
        const size_t ne = hs[d * kHdrWords];
        if (ne) HIP_OK(hipMemcpyAsync(sendp + at, p.outbox + (size_t)d * p.out_cap, ne * sizeof(Entry), hipMemcpyDeviceToDevice, st));
        at += pad8(ne * sizeof(Entry));
        if (q_bytes) HIP_OK(hipMemcpyAsync(sendp + at, w.queries + q_end[r], q_bytes, hipMemcpyDeviceToDevice, st));
        at += q_bytes;
        if (j_bytes) HIP_OK(hipMemcpyAsync(sendp + at, w.joins + j_end[r], j_bytes, hipMemcpyDeviceToDevice, st));
        at += j_bytes;
      }
      X.alltoallv(sendp, sb, recvp, rb, st);
      // 3. import the peers' queries and joins, then ingest their entries
      at = 0;
      std::vector<std::pair<size_t, uint32_t>> ents;  // (offset, count) per peer
      for (uint32_t s = 0; s < W; ++s) {
        if (s == r) continue;
        const uint64_t* h = &rh[s * kHdrWords];
        ents.push_back({at, (uint32_t)h[0]});
        at += pad8(h[0] * sizeof(Entry));
        if (h[2]) HIP_OK(hipMemcpyAsync(w.queries + h[1], recvp + at, h[2] * sizeof(DevQuery), hipMemcpyDeviceToDevice, st));
        at += h[2] * sizeof(DevQuery);
        if (h[4]) {
          HIP_OK(hipMemcpyAsync(w.joins + h[3], recvp + at, h[4] * sizeof(DevJoin), hipMemcpyDeviceToDevice, st));
          hipLaunchKernelGGL(k_part_adopt_joins, dim3(grid_for(h[4])), dim3(kBlock), 0, st, w.queries, w.joins + h[3],
                             (uint32_t)h[4], c.query_cap, w.ctr);
        }
        at += h[4] * sizeof(DevJoin);
        q_end[s] = (uint32_t)(h[1] + h[2]);
        j_end[s] = (uint32_t)(h[3] + h[4]);
      }
      for (auto& [off, cnt] : ents)
        if (cnt)
          hipLaunchKernelGGL(k_part_ingest, dim3(grid_for(cnt)), dim3(kBlock), 0, st, c,
                             reinterpret_cast<const Entry*>(recvp + off), cnt);
      HIP_OK(hipGetLastError());
    }
    q_end[r] = my_q;
    j_end[r] = my_j;
    // 4. flag planes over every allocated query, OR-ed over the ranks; then the resolve
    PartRanges R{};
    R.n = 0;
    uint32_t M = 0;
    auto add = [&](uint32_t lo, uint32_t hi) {
      R.lo[R.n] = lo;
      R.at[R.n] = M;
      ++R.n;
      M += hi - lo;
    };
    add(0, n);
    for (uint32_t s = 0; s < W; ++s)
      if (q_end[s] > q_base[s]) add(q_base[s], q_end[s]);
    R.at[R.n] = M;
    uint8_t* fl = p.flags.want(4 * (size_t)M + 1);
    hipLaunchKernelGGL(k_part_export, dim3(grid_for((uint64_t)M + 1)), dim3(kBlock), 0, st, c, R, M, fl);
    HIP_OK(hipGetLastError());
    X.allreduce_max(fl, 4 * (uint64_t)M + 1, st);
    uint8_t* h_over = reinterpret_cast<uint8_t*>(p.h_cnt);
    HIP_OK(hipMemcpyAsync(h_over, fl + 4 * (size_t)M, 1, hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(k_part_import, dim3(grid_for(M)), dim3(kBlock), 0, st, c, R, M, fl);
    for (uint32_t k = 0; k < R.n; ++k) {
      const uint32_t lo = R.lo[k], hi = lo + (R.at[k + 1] - R.at[k]);
      hipLaunchKernelGGL(k_resolve_range, dim3(std::min<uint32_t>(1024, grid_for(hi - lo))), dim3(kBlock), 0, st, c, lo, hi);
    }
    hipLaunchKernelGGL(k_level_end, dim3(1), dim3(1), 0, st, w.ctr);
    hipLaunchKernelGGL(k_part_open, dim3(grid_for(n)), dim3(kBlock), 0, st, c, n, p.out_cnt + W);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(p.h_ctr, w.ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(p.h_out + W, p.out_cnt + W, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    ++levels;
    if (h_over[0]) return false;  // every rank: the overflow byte was reduced
    n_cur = p.h_ctr->last_next;
    cur ^= 1;
    if (p.h_out[W] == 0) break;
  }
  hipLaunchKernelGGL(k_final, dim3(grid_for(n)), dim3(kBlock), 0, st, w.queries, n, w.item_err, d_perm, d_err, w.ctr);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(p.h_ctr, w.ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (p.h_ctr->overflow & 32u) throw Error(GCK_E_DEVICE, "engine invariant violated: undecided check");
  add_counters(e, w, *p.h_ctr);
  std::lock_guard<std::mutex> sl(e.stats_mu);
  e.stats.levels += levels;
  e.stats.queries += n;
  return true;
}

// What the label join left (n_left checks in p.left), through the level loop in chunks small enough
// for the query ids; a chunk that overflows runs again split in half (every rank alike).
static void part_leftovers(Engine& e, const Xport& X, Workspace& w, PartState& p, uint32_t n_left, int64_t now_us,
                           hipStream_t st) {
  const Ctx c0 = make_ctx(e, w, now_us, st);
  uint32_t chunk = std::max<uint32_t>(1, c0.query_cap / 4);
  for (uint32_t pos = 0; pos < n_left;) {
    const uint32_t len = std::min(chunk, n_left - pos);
    if (part_loop(e, X, w, p, p.left + pos, len, now_us, p.lperm + pos, p.lerr + pos, st)) {
      pos += len;
      continue;
    }
    {
      std::lock_guard<std::mutex> sl(e.stats_mu);
      e.stats.retries++;
    }
    if (len == 1) throw Error(GCK_E_CAPACITY, "partitioned check: one check overflows the workspace");
    chunk = std::max<uint32_t>(1, len / 2);
  }
}

// One partitioned batch: the label join, then the level loop over what it left.
static void part_run(Engine& e, const Xport& X, const gck_item* d_items, size_t n, int64_t now_us, uint8_t* d_perm,
                     int32_t* d_err, hipStream_t st) {
  part_require(e);
  HIP_OK(hipSetDevice(e.device));
  const uint32_t W = e.part_world, r = e.part_rank;
  Workspace& w = part_workspace(e);
  if (n > w.max_batch) throw Error(GCK_E_CAPACITY, "partitioned batch above max_batch");
  // one partitioned batch at a time on the engine's partition workspace, its state created and its
  // buffers grown under the same lock (two concurrent callers must not free what the other's
  // kernels still use)
  std::lock_guard<std::mutex> batch_lock(w.m);
  PartState& p = part_bufs(e, w, n);
  if (n == 0) return;
  PhaseClock pc("part_check");
  // one evaluation time for every rank: rank 0's clock when the caller gave none
  if (now_us == 0) {
    now_us = wall_now_us();
    if (W > 1) {
      std::vector<uint64_t> sb(W, 0), rb(W, 0);
      if (r == 0)
        for (uint32_t d = 1; d < W; ++d) sb[d] = 8;
      else
        rb[0] = 8;
      uint8_t* b = p.misc.want(8 * (size_t)W + 8);
      if (r == 0)
        for (uint32_t d = 1; d < W; ++d) HIP_OK(hipMemcpyAsync(b + 8 * (d - 1), &now_us, 8, hipMemcpyHostToDevice, st));
      X.alltoallv(b, sb, b + 8 * (size_t)W, rb, st);
      if (r != 0) HIP_OK(hipMemcpyAsync(&now_us, b + 8 * (size_t)W, 8, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
    }
  }
  const DeviceSnapshot& ds = *e.dev;
  uint32_t n_left = (uint32_t)n;
  // GCK_FLAG_PROFILE: the join's own kernels timed by their events (stats bundle_ms /
  // bundle_launches, the bench's roofline): k_label_join on one rank, k_pj_pack + k_pj_decide on
  // several (the exchange between them not included)
  const bool prof = (e.cfg.flags & GCK_FLAG_PROFILE) != 0;
  float join_ms = -1.f;
  if (W == 1 && ds.d_lj) {
    // one rank owns every slot: the label join kernel itself (labels.inc k_label_join); its
    // leftovers (any order: no other rank to agree with) through the level loop
    HIP_OK(hipMemsetAsync(p.cnt, 0, 4, st));
    LjArgs j{};
    j.items = d_items;
    j.n = (uint32_t)n;
    j.out_perm = d_perm;
    j.out_err = d_err;
    j.deferred = p.idx;
    j.n_deferred = p.cnt;
    lj_table_args(ds, j);
    lj_launch(lj_variant(ds, false), j, (uint32_t)n, st, prof ? w.ev0 : nullptr, prof ? w.ev1 : nullptr);
    HIP_OK(hipMemcpyAsync(p.h_cnt, p.cnt, 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (prof) HIP_OK(hipEventElapsedTime(&join_ms, w.ev0, w.ev1));
    n_left = p.h_cnt[0];
    if (n_left > n) throw Error(GCK_E_DEVICE, "engine invariant violated: leftover count");
    add_join_stats(e, n, n_left);
    if (n_left) {
      hipLaunchKernelGGL(k_gather, dim3(grid_for(n_left)), dim3(kBlock), 0, st, d_items, p.idx, n_left, p.left);
      HIP_OK(hipGetLastError());
    }
  } else if (W == 1) {
    HIP_OK(hipMemcpyAsync(p.left, d_items, n * sizeof(gck_item), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_iota, dim3(grid_for(n)), dim3(kBlock), 0, st, p.idx, (uint32_t)n);
    HIP_OK(hipGetLastError());
  } else {
    // 1. the label join: (check, user slot) records to the owners of the resources, decided there
    HIP_OK(hipMemsetAsync(d_perm, 0, n, st));
    HIP_OK(hipMemsetAsync(d_err, 0, n * 4, st));
    if (ds.d_lj) {
      HIP_OK(hipMemsetAsync(p.cnt, 0, (W + 1) * 4, st));
      if (prof) HIP_OK(hipEventRecord(w.pev[0], st));
      hipLaunchKernelGGL(k_pj_pack, dim3(grid_for(n)), dim3(kBlock), 0, st, lj_tab(ds), d_items, (uint32_t)n, r, W, p.out,
                         (uint32_t)p.cap, p.cnt);
      HIP_OK(hipGetLastError());
      if (prof) HIP_OK(hipEventRecord(w.pev[1], st));
      HIP_OK(hipMemcpyAsync(p.h_cnt, p.cnt, (W + 1) * 4, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      std::vector<uint64_t> sc(W), sb(W, 0), rb(W, 0);
      for (uint32_t d = 0; d < W; ++d) {
        sc[d] = std::min<uint64_t>(p.h_cnt[d], p.cap);  // (records past a region's end were not written)
        if (d != r) sb[d] = rb[d] = 8;
      }
      // the records' counts (8 B per peer), then the records (kPjRecWords words each)
      uint8_t* cb = p.hdr.want(2 * (size_t)W * 8);
      {
        size_t k = 0;
        for (uint32_t d = 0; d < W; ++d)
          if (d != r) p.h_hdr[k++] = sc[d];
      }
      HIP_OK(hipMemcpyAsync(cb, p.h_hdr, (W - 1) * 8, hipMemcpyHostToDevice, st));
      X.alltoallv(cb, sb, cb + (size_t)W * 8, rb, st);
      HIP_OK(hipMemcpyAsync(p.h_hdr + W, cb + (size_t)W * 8, (W - 1) * 8, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      std::vector<uint64_t> rc(W, 0);
      {
        size_t k = 0;
        for (uint32_t s = 0; s < W; ++s)
          if (s != r) rc[s] = p.h_hdr[W + k++];
      }
      constexpr size_t kRec = kPjRecWords * 4;
      size_t s_total = 0, r_total = 0;
      for (uint32_t d = 0; d < W; ++d) {
        sb[d] = d == r ? 0 : sc[d] * kRec;
        rb[d] = d == r ? 0 : rc[d] * kRec;
        s_total += sb[d];
        r_total += rb[d];
      }
      uint8_t* sendp = p.send.want(std::max<size_t>(s_total, 8));
      uint8_t* recvp = p.recv.want(std::max<size_t>(r_total, 8));
      size_t at = 0;
      for (uint32_t d = 0; d < W; ++d) {
        if (d == r || !sb[d]) continue;
        HIP_OK(hipMemcpyAsync(sendp + at, p.out + (size_t)d * p.cap * kPjRecWords, sb[d], hipMemcpyDeviceToDevice, st));
        at += sb[d];
      }
      X.alltoallv(sendp, sb, recvp, rb, st);
      // this rank's own records in place, the received ones after them
      auto decide = [&](const uint32_t* recs, size_t cnt) {
        if (!cnt) return;
        if (ds.lj.bits == 24)
          hipLaunchKernelGGL(k_pj_decide<24>, dim3(grid_for(cnt)), dim3(kBlock), 0, st, lj_tab(ds), d_items, (uint32_t)n,
                             ds.lj.sw, W, recs, (uint32_t)cnt, nullptr, d_perm, d_err);
        else
          hipLaunchKernelGGL(k_pj_decide<32>, dim3(grid_for(cnt)), dim3(kBlock), 0, st, lj_tab(ds), d_items, (uint32_t)n,
                             ds.lj.sw, W, recs, (uint32_t)cnt, nullptr, d_perm, d_err);
        HIP_OK(hipGetLastError());
      };
      if (prof) HIP_OK(hipEventRecord(w.pev[2], st));
      decide(p.out + (size_t)r * p.cap * kPjRecWords, sc[r]);
      decide(reinterpret_cast<const uint32_t*>(recvp), r_total / kRec);
      if (prof) {
        HIP_OK(hipEventRecord(w.pev[3], st));
        HIP_OK(hipEventSynchronize(w.pev[3]));
        float a = 0.f, b = 0.f;
        HIP_OK(hipEventElapsedTime(&a, w.pev[0], w.pev[1]));
        HIP_OK(hipEventElapsedTime(&b, w.pev[2], w.pev[3]));
        join_ms = a + b;
      }
      // every rank every answer (a check is decided on one rank only; the others hold 0)
      X.allreduce_max(d_perm, n, st);
    }
    // 2. what no rank decided, in batch order on every rank
    const uint32_t nb = grid_for(n);
    hipLaunchKernelGGL(k_pj_bcount, dim3(nb), dim3(kBlock), 0, st, d_perm, (uint32_t)n, p.flag);
    hipLaunchKernelGGL(k_pj_bscan, dim3(1), dim3(64), 0, st, p.flag, nb, p.pos);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(p.h_cnt, p.pos, 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    n_left = p.h_cnt[0];
    if (n_left > n) throw Error(GCK_E_DEVICE, "engine invariant violated: leftover count");
    add_join_stats(e, ds.d_lj ? n : n_left, n_left);
    if (n_left) {
      hipLaunchKernelGGL(k_pj_place, dim3(nb), dim3(kBlock), 0, st, d_items, d_perm, (uint32_t)n, p.flag, p.idx, p.left);
      HIP_OK(hipGetLastError());
    }
  }
  pc.mark("join");
  if (pc.on) {
    char b[48];
    snprintf(b, sizeof(b), " left=%u", n_left);
    pc.line += b;
  }
  {
    std::lock_guard<std::mutex> sl(e.stats_mu);
    e.stats.batches++;
    if (!n_left) e.stats.queries += n;
    if (join_ms >= 0.f) {
      e.stats.bundle_ms += join_ms;
      e.stats.bundle_launches++;
    }
  }
  if (!n_left) return;
  part_leftovers(e, X, w, p, n_left, now_us, st);
  hipLaunchKernelGGL(k_scatter, dim3(grid_for(n_left)), dim3(kBlock), 0, st, p.idx, n_left, p.lperm, p.lerr, d_perm, d_err);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(st));
  pc.mark("loop");
}

// ---- the RCCL transport (gck_part_check) ---------------------------------------------------------

#define RCCL_OK(x)                                                                              \
  do {                                                                                          \
    ncclResult_t r_ = (x);                                                                      \
    if (r_ != ncclSuccess) throw Error(GCK_E_DEVICE, std::string("RCCL error: ") + ncclGetErrorString(r_)); \
  } while (0)

struct RcclCtx {
  ncclComm_t comm;
  int rank, world;
};

// grouped ncclSend / ncclRecv, one pair per peer with bytes to move
static int rccl_alltoallv(void* ctx, const void* send, const uint64_t* sb, void* recv, const uint64_t* rb, void* stream) {
  const RcclCtx& x = *static_cast<const RcclCtx*>(ctx);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint8_t* s = static_cast<const uint8_t*>(send);
  uint8_t* d = static_cast<uint8_t*>(recv);
  size_t s_at = 0, r_at = 0, self_s = 0, self_r = 0;
  if (ncclGroupStart() != ncclSuccess) return -1;
  for (int p = 0; p < x.world; ++p) {
    if (p == x.rank) {
      self_s = s_at, self_r = r_at;
    } else {
      if (sb[p] && ncclSend(s + s_at, sb[p], ncclUint8, p, x.comm, st) != ncclSuccess) return (void)ncclGroupEnd(), -1;
      if (rb[p] && ncclRecv(d + r_at, rb[p], ncclUint8, p, x.comm, st) != ncclSuccess) return (void)ncclGroupEnd(), -1;
    }
    s_at += sb[p];
    r_at += rb[p];
  }
  if (ncclGroupEnd() != ncclSuccess) return -1;
  const uint64_t self = std::min(sb[x.rank], rb[x.rank]);
  if (self && hipMemcpyAsync(d + self_r, s + self_s, self, hipMemcpyDeviceToDevice, st) != hipSuccess) return -1;
  return 0;
}

static int rccl_allreduce_max_u8(void* ctx, void* buf, uint64_t n, void* stream) {
  const RcclCtx& x = *static_cast<const RcclCtx*>(ctx);
  return ncclAllReduce(buf, buf, n, ncclUint8, ncclMax, x.comm, static_cast<hipStream_t>(stream)) == ncclSuccess ? 0 : -1;
}

void part_unique_id(uint8_t* out) {
  ncclUniqueId id;
  RCCL_OK(ncclGetUniqueId(&id));
  std::memcpy(out, id.internal, NCCL_UNIQUE_ID_BYTES);
}

void part_comm_free(Engine& e) {
  if (!e.part_comm) return;
  (void)hipSetDevice(e.device);
  auto* x = static_cast<RcclCtx*>(e.part_comm);
  (void)ncclCommDestroy(x->comm);
  delete x;
  e.part_comm = nullptr;
}

void part_init(Engine& e, const uint8_t* bytes) {
  part_require(e);
  HIP_OK(hipSetDevice(e.device));
  part_comm_free(e);
  ncclUniqueId id;
  std::memcpy(id.internal, bytes, NCCL_UNIQUE_ID_BYTES);
  ncclComm_t comm = nullptr;
  RCCL_OK(ncclCommInitRank(&comm, (int)e.part_world, id, (int)e.part_rank));
  e.part_comm = new RcclCtx{comm, (int)e.part_rank, (int)e.part_world};
}

void part_check(Engine& e, const gck_item* d_items, size_t n, int64_t now_us, uint8_t* d_perm, int32_t* d_err,
                void* stream) {
  part_require(e);
  if (!e.part_comm) throw Error(GCK_E_STATE, "no RCCL communicator (gck_part_init)");
  const gck_transport t{e.part_comm, rccl_alltoallv, rccl_allreduce_max_u8};
  const Xport X{&t, e.part_rank, e.part_world};
  part_run(e, X, d_items, n, now_us, d_perm, d_err, (hipStream_t)stream);
}

void part_check_with(Engine& e, const gck_transport& t, const gck_item* d_items, size_t n, int64_t now_us,
                     uint8_t* d_perm, int32_t* d_err, void* stream) {
  if (e.part_world > 1 && (!t.alltoallv || !t.allreduce_max_u8))
    throw Error(GCK_E_INVALID_ARGUMENT, "transport without functions");
  const Xport X{&t, e.part_rank, e.part_world};
  part_run(e, X, d_items, n, now_us, d_perm, d_err, (hipStream_t)stream);
}

// ---- object names on a partitioned graph (SURVEY §8e: owner(obj) = hash(type, id) mod G) -------
//
// Ownership is decided from the name, before anything is interned: the owner of (type, name) is
// hash(type, name) mod world, and only the owner gives the name an id — local * world + owner, its
// local counter in order — so that part_owner(id) = id mod world names the same rank the engine's
// device side uses, and every rank holds the same id for a name. A rank interns the names of the
// objects it owns and asks the owners for the names its own tuples and checks reference (the
// subjects of its rows, the replicated hub hierarchy): with the export stream
// (client/client.go:472-499) read by every rank, its interner holds about 1/world of the objects
// plus the hubs, instead of all of them.

static uint64_t name_hash(uint16_t type, const char* s, size_t len) {
  uint64_t h = 1469598103934665603ull;  // FNV-1a over the type (2 bytes LE) and the name's bytes
  h = (h ^ (type & 0xFFu)) * 1099511628211ull;
  h = (h ^ (type >> 8)) * 1099511628211ull;
  for (size_t i = 0; i < len; ++i) h = (h ^ (uint8_t)s[i]) * 1099511628211ull;
  h ^= h >> 33;  // (finalised: the low bits pick the rank)
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  return h;
}

uint32_t part_owner_name(uint16_t type, const char* s, size_t len, uint32_t world) {
  return world <= 1 ? 0u : (uint32_t)(name_hash(type, s, len) % world);
}

// Host byte blocks to every rank and back through the transport's all-to-all (device staging:
// the transport moves device memory): out[d] to rank d, the result's [s] from rank s. A rank's
// own block stays here (the transport is passed 0 bytes for it, include/gck.h).
static std::vector<std::vector<uint8_t>> part_exchange(const Xport& X, const std::vector<std::vector<uint8_t>>& out) {
  const uint32_t W = X.world, r = X.rank;
  std::vector<uint64_t> sb(W), rb(W, 8), s8(W, 8);
  for (uint32_t d = 0; d < W; ++d) sb[d] = d == r ? 0 : out[d].size();
  s8[r] = 0;
  std::vector<void*> tmp;
  std::vector<std::vector<uint8_t>> in(W);
  in[r] = out[r];
  if (W <= 1) return in;
  try {
    uint64_t* d_sz = dalloc<uint64_t>(tmp, 2 * (size_t)W);
    // (each rank the size of its block for every other rank: 8 bytes to each, at the receiver's
    // position in rank order; the own slot is not sent)
    std::vector<uint64_t> packed;
    for (uint32_t d = 0; d < W; ++d)
      if (d != r) packed.push_back(sb[d]);
    HIP_OK(hipMemcpy(d_sz, packed.data(), 8 * packed.size(), hipMemcpyHostToDevice));
    X.alltoallv(d_sz, s8, d_sz + W, s8, nullptr);
    std::vector<uint64_t> got_sz(W - 1);
    HIP_OK(hipStreamSynchronize(nullptr));
    HIP_OK(hipMemcpy(got_sz.data(), d_sz + W, 8 * got_sz.size(), hipMemcpyDeviceToHost));
    for (uint32_t s = 0, k = 0; s < W; ++s) rb[s] = s == r ? 0 : got_sz[k++];
    uint64_t ts = 0, tr = 0;
    for (uint32_t d = 0; d < W; ++d) ts += sb[d], tr += rb[d];
    uint8_t* d_buf = dalloc<uint8_t>(tmp, std::max<uint64_t>(1, ts + tr));
    std::vector<uint8_t> flat;
    flat.reserve(ts);
    for (uint32_t d = 0; d < W; ++d)
      if (d != r) flat.insert(flat.end(), out[d].begin(), out[d].end());
    if (ts) HIP_OK(hipMemcpy(d_buf, flat.data(), ts, hipMemcpyHostToDevice));
    X.alltoallv(d_buf, sb, d_buf + ts, rb, nullptr);
    HIP_OK(hipStreamSynchronize(nullptr));
    std::vector<uint8_t> got(tr);
    if (tr) HIP_OK(hipMemcpy(got.data(), d_buf + ts, tr, hipMemcpyDeviceToHost));
    uint64_t at = 0;
    for (uint32_t s = 0; s < W; ++s) {
      if (s == r) continue;
      in[s].assign(got.begin() + at, got.begin() + at + rb[s]);
      at += rb[s];
    }
  } catch (...) {
    free_list(tmp);
    throw;
  }
  free_list(tmp);
  return in;
}

static void name_store(TypeInterner& ti, const std::string& name, uint32_t id) {
  ti.ids.emplace(name, id);
  ti.rev.emplace(id, name);
}

// Collective: every rank calls it (the same number of times, the same `create`) with its own
// names. out[i] = the id of (types[i], names[i]) — GCK_ID_WILDCARD for "*", GCK_ID_ABSENT for a
// name its owner does not know (create false). With create, every rank's object counts become
// world x the largest local count (the id space).
void part_intern(Engine& e, const gck_transport& t, const uint16_t* types, const char* const* names,
                 const uint32_t* lens, size_t n, bool create, uint32_t* out) {
  part_require(e);
  HIP_OK(hipSetDevice(e.device));
  const uint32_t W = e.part_world, r = e.part_rank;
  const Xport X{&t, r, W};
  if (W > 1 && !t.alltoallv) throw Error(GCK_E_INVALID_ARGUMENT, "transport without functions");
  const Schema& sc = *e.schema;
  std::vector<std::vector<uint8_t>> req(W);
  std::vector<std::vector<size_t>> req_at(W);  // the out index each request answers
  std::vector<std::pair<size_t, size_t>> alias;  // (i, the index of the same name's request)
  std::unordered_map<std::string, size_t> asked;
  std::string key;
  for (size_t i = 0; i < n; ++i) {
    if (types[i] >= sc.types.size()) throw Error(GCK_E_INVALID_ARGUMENT, "unknown type id");
    const std::string_view nm(names[i] ? names[i] : "", names[i] ? lens[i] : 0);
    if (nm == "*") {
      out[i] = kWildcard;
      continue;
    }
    TypeInterner& ti = e.interner[types[i]];
    auto it = ti.ids.find(std::string(nm));
    if (it != ti.ids.end()) {
      out[i] = it->second;
      continue;
    }
    key.assign(reinterpret_cast<const char*>(&types[i]), 2);
    key.append(nm);
    auto a = asked.find(key);
    if (a != asked.end()) {
      alias.push_back({i, a->second});
      continue;
    }
    asked.emplace(key, i);
    const uint32_t d = part_owner_name(types[i], nm.data(), nm.size(), W);
    std::vector<uint8_t>& b = req[d];
    const uint32_t len = (uint32_t)nm.size();
    const size_t o = b.size();
    b.resize(o + 8 + ((len + 3) & ~3u), 0);
    std::memcpy(b.data() + o, &types[i], 2);
    std::memcpy(b.data() + o + 4, &len, 4);
    std::memcpy(b.data() + o + 8, nm.data(), len);
    req_at[d].push_back(i);
  }
  // as the owner: every rank's requests in rank order (this rank's own among them)
  const std::vector<std::vector<uint8_t>> in = part_exchange(X, req);
  std::vector<std::vector<uint8_t>> rep(W);
  for (uint32_t s = 0; s < W; ++s) {
    const std::vector<uint8_t>& b = in[s];
    for (size_t o = 0; o + 8 <= b.size();) {
      uint16_t ty = 0;
      uint32_t len = 0;
      std::memcpy(&ty, b.data() + o, 2);
      std::memcpy(&len, b.data() + o + 4, 4);
      if (ty >= sc.types.size() || o + 8 + len > b.size()) throw Error(GCK_E_DEVICE, "partition transport: bad name record");
      std::string nm(reinterpret_cast<const char*>(b.data() + o + 8), len);
      o += 8 + ((len + 3) & ~3u);
      TypeInterner& ti = e.interner[ty];
      uint32_t id = kAbsent;
      auto it = ti.ids.find(nm);
      if (it != ti.ids.end()) {
        id = it->second;
      } else if (create) {
        const uint64_t g = (uint64_t)ti.local * W + r;
        if (g >= kAbsent) throw Error(GCK_E_CAPACITY, "too many objects of one type");
        ++ti.local;
        id = (uint32_t)g;
        name_store(ti, nm, id);
      }
      const size_t q = rep[s].size();
      rep[s].resize(q + 4);
      std::memcpy(rep[s].data() + q, &id, 4);
    }
  }
  const std::vector<std::vector<uint8_t>> back = part_exchange(X, rep);
  for (uint32_t d = 0; d < W; ++d) {
    if (back[d].size() != 4 * req_at[d].size()) throw Error(GCK_E_DEVICE, "partition transport: bad name reply");
    for (size_t k = 0; k < req_at[d].size(); ++k) {
      const size_t i = req_at[d][k];
      uint32_t id = kAbsent;
      std::memcpy(&id, back[d].data() + 4 * k, 4);
      out[i] = id;
      if (id != kAbsent && d != r) name_store(e.interner[types[i]], std::string(names[i], lens[i]), id);
    }
  }
  for (auto& [i, j] : alias) out[i] = out[j];
  if (!create) return;
  // the id space: world x the largest local count of each type (every rank the same)
  const size_t T = sc.types.size();
  std::vector<std::vector<uint8_t>> loc(W, std::vector<uint8_t>(4 * T));
  for (uint32_t d = 0; d < W; ++d)
    for (size_t ty = 0; ty < T; ++ty) std::memcpy(loc[d].data() + 4 * ty, &e.interner[ty].local, 4);
  const std::vector<std::vector<uint8_t>> all = part_exchange(X, loc);
  for (size_t ty = 0; ty < T; ++ty) {
    uint32_t mx = 0;
    for (uint32_t s = 0; s < W; ++s) {
      uint32_t v = 0;
      if (all[s].size() >= 4 * (ty + 1)) std::memcpy(&v, all[s].data() + 4 * ty, 4);
      mx = std::max(mx, v);
    }
    const uint64_t c = (uint64_t)mx * W;
    if (c >= kAbsent) throw Error(GCK_E_CAPACITY, "too many objects of one type");
    e.interner[ty].count = std::max(e.interner[ty].count, (uint32_t)c);
  }
}

// Collective: the export stream's text on a partitioned graph (every rank the same text, between
// gck_begin_snapshot and gck_commit_snapshot). Each rank keeps what part_keep gives it — decided
// by the names' owners before anything is interned — and interns the names of those tuples only.
void part_add_tuples_text(Engine& e, const gck_transport& t, const char* text, size_t len) {
  part_require(e);
  const uint32_t W = e.part_world, r = e.part_rank;
  std::vector<TupleNames> all = parse_tuples_text(e, text, len);  // (caveat instances: every line, every rank)
  std::vector<uint16_t> types;
  std::vector<const char*> nms;
  std::vector<uint32_t> lens;
  std::vector<size_t> kept;
  for (size_t k = 0; k < all.size(); ++k) {
    const TupleNames& p = all[k];
    const bool wild = p.sid == "*";
    const uint32_t o_res = part_owner_name(p.rt, p.rid.data(), p.rid.size(), W);
    const uint32_t o_sub = wild ? W : part_owner_name(p.st, p.sid.data(), p.sid.size(), W);
    const bool hub = p.rel < e.part_hub_rel.size() && e.part_hub_rel[p.rel];
    const bool keep = hub ? (p.srel != kEllipsis || wild || o_sub == r) : o_res == r;  // (part_keep)
    if (!keep) continue;
    kept.push_back(k);
    types.push_back(p.rt);
    nms.push_back(p.rid.data());
    lens.push_back((uint32_t)p.rid.size());
    types.push_back(p.st);
    nms.push_back(p.sid.data());
    lens.push_back((uint32_t)p.sid.size());
  }
  std::vector<uint32_t> ids(types.size());
  part_intern(e, t, types.data(), nms.data(), lens.data(), types.size(), true, ids.data());
  for (size_t q = 0; q < kept.size(); ++q) {
    const TupleNames& p = all[kept[q]];
    gck_tuple tu{};
    tu.resource_type = p.rt;
    tu.relation = p.rel;
    tu.resource_id = ids[2 * q];
    tu.subject_type = p.st;
    tu.subject_relation = p.srel;
    tu.subject_id = ids[2 * q + 1];
    tu.caveat = p.cav;
    tu.expires_at_us = p.exp;
    stage_tuple(e, tu);  // (validated; part_keep by id agrees: id mod world is the name's owner)
  }
}
