// lookup.inc — LookupResources / LookupSubjects on the check engine (included by engine.hip).
//
// SURVEY.md §8f3: Client.LookupResources (client/client.go:508-552) streams the ids of the
// objects of a type on which a subject has a permission; Client.LookupSubjects (:560-599) the
// ids of the subjects of a type that have a permission on one object. Both are answered here by
// checking every candidate on the device — the objects of the resource type, or the subjects of
// the subject type — through the same bundle / grid-wide stages as CheckBulkPermissions, with
// the candidate items generated and the answers compacted on the device, so the host sees only
// the matching ids. A candidate matches when its check is HAS or CONDITIONAL (SpiceDB returns
// both, flagged; the client yields the ids of both). The candidate sweep costs one check per
// object of the type: a 64K-candidate chunk per batch of the check path.

// Items of one candidate chunk [base, base + n): either the resource id varies (`vary_res`) or
// the subject id does.
__global__ void __launch_bounds__(kBlock) k_lookup_items(gck_item proto, uint32_t base, uint32_t n, bool vary_res,
                                                         gck_item* __restrict__ out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  gck_item it = proto;
  if (vary_res) it.resource_id = base + i;
  else it.subject_id = base + i;
  out[i] = it;
}

// Matching candidates of a chunk, appended in any order (the host sorts): id and permissionship;
// a per-item error (max depth) is flagged for the whole request.
__global__ void __launch_bounds__(kBlock) k_lookup_collect(const uint8_t* __restrict__ perm,
                                                           const int32_t* __restrict__ err, uint32_t base, uint32_t n,
                                                           uint32_t* __restrict__ out_ids, uint8_t* __restrict__ out_perm,
                                                           unsigned* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  if (err[i] != GCK_ITEM_OK) {
    atomicMax(&cnt[1], (unsigned)err[i]);
    return;
  }
  const uint8_t p = perm[i];
  if (p != GCK_PERM_HAS && p != GCK_PERM_CONDITIONAL) return;
  const unsigned k = atomicAdd(&cnt[0], 1u);
  out_ids[k] = base + i;
  out_perm[k] = p;
}

// Sweeps candidate ids [0, n_candidates) of `proto` (the varying id is overwritten) and returns
// the matching (id, permissionship) pairs, ascending by id.
void device_lookup(Engine& e, Workspace& w, const gck_item& proto, bool vary_res, uint32_t n_candidates,
                   int64_t now_us, std::vector<uint32_t>& ids, std::vector<uint8_t>& perms) {
  HIP_OK(hipSetDevice(e.device));
  std::lock_guard<std::mutex> lk(w.m);
  stage_caveats(w, CavCall(), w.stream);
  if (now_us == 0) now_us = wall_now_us();
  if (!w.lk_ids) {
    w.lk_ids = dalloc<uint32_t>(w.allocs, w.max_batch);
    w.lk_perm = dalloc<uint8_t>(w.allocs, w.max_batch);
    w.lk_cnt = dalloc<unsigned>(w.allocs, 2);
    HIP_OK(hipStreamSynchronize(nullptr));  // pool allocations are ordered on the null stream
  }
  float ms = 0.f;
  std::vector<std::pair<uint32_t, uint8_t>> found;
  unsigned h_cnt[2] = {0, 0};
  for (uint32_t base = 0; base < n_candidates; base += (uint32_t)w.max_batch) {
    const uint32_t n = (uint32_t)std::min<size_t>(n_candidates - base, w.max_batch);
    hipLaunchKernelGGL(k_lookup_items, dim3(grid_for(n)), dim3(kBlock), 0, w.stream, proto, base, n, vary_res,
                       w.d_items);
    HIP_OK(hipGetLastError());
    check_range(e, w, w.d_items, n, now_us, w.d_perm, w.d_err, w.stream, &ms);
    HIP_OK(hipMemsetAsync(w.lk_cnt, 0, 2 * sizeof(unsigned), w.stream));
    hipLaunchKernelGGL(k_lookup_collect, dim3(grid_for(n)), dim3(kBlock), 0, w.stream, w.d_perm, w.d_err, base, n,
                       w.lk_ids, w.lk_perm, w.lk_cnt);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h_cnt, w.lk_cnt, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, w.stream));
    HIP_OK(hipStreamSynchronize(w.stream));
    if (h_cnt[1] != 0) {
      throw Error(GCK_E_INVALID_ARGUMENT,
                  h_cnt[1] == GCK_ITEM_ERR_MAX_DEPTH ? "max depth exceeded: this usually indicates a recursive or too "
                                                       "deep data dependency"
                                                     : "lookup failed: per-item error " + std::to_string(h_cnt[1]));
    }
    if (h_cnt[0]) {
      std::vector<uint32_t> ci(h_cnt[0]);
      std::vector<uint8_t> cp(h_cnt[0]);
      HIP_OK(hipMemcpyAsync(ci.data(), w.lk_ids, ci.size() * 4, hipMemcpyDeviceToHost, w.stream));
      HIP_OK(hipMemcpyAsync(cp.data(), w.lk_perm, cp.size(), hipMemcpyDeviceToHost, w.stream));
      HIP_OK(hipStreamSynchronize(w.stream));
      for (size_t k = 0; k < ci.size(); ++k) found.emplace_back(ci[k], cp[k]);
    }
  }
  std::sort(found.begin(), found.end());
  ids.resize(found.size());
  perms.resize(found.size());
  for (size_t k = 0; k < found.size(); ++k) {
    ids[k] = found[k].first;
    perms[k] = found[k].second;
  }
  std::lock_guard<std::mutex> sl(e.stats_mu);
  e.stats.kernel_ms = ms;
}

// The per-item error that fails a lookup among candidates: device_lookup's code and message (that
// function and device_lookup_subjects, left as they are, keep their own text of it).
[[noreturn]] static void lookup_item_error(unsigned code) {
  throw Error(GCK_E_INVALID_ARGUMENT,
              code == GCK_ITEM_ERR_MAX_DEPTH ? "max depth exceeded: this usually indicates a recursive or too "
                                               "deep data dependency"
                                             : "lookup failed: per-item error " + std::to_string(code));
}

// A lookup among the caller's candidates (engine.hpp): one list request — the candidates' 4-B ids,
// or the range of a whole type — through the compact path, so that its chunks are in flight over
// both workspaces and each costs one join dispatch; the 2-bit plane comes back through the
// workspaces' pinned result staging and is scanned here, zero words skipped. A candidate with a
// per-item error fails the call as device_lookup fails: the largest code of the first chunk that
// has one — the same chunks as that sweep's when max_batch is a multiple of 32 (it steps by
// max_batch, the compact path by max_batch & ~31), so the same code.
void device_lookup_among(Engine& e, Workspace* w0, Workspace* w1, const CompactReq& req, int64_t now_us,
                         std::vector<uint32_t>& ids, std::vector<uint8_t>& perms) {
  ids.clear();
  perms.clear();
  if (req.n == 0) return;
  HIP_OK(hipSetDevice(e.device));
  if (now_us == 0) now_us = wall_now_us();
  std::vector<uint64_t> plane((req.n + 31) / 32);
  CompactReq q = req;
  q.packed = plane.data();
  std::vector<gck_item_error> errs;  // (every chunk's, whole: no list of the caller's bounds them)
  const size_t mb = compact_chunks(e, w0, w1, q, now_us, CavCall(), errs);
  if (!errs.empty()) {
    size_t chunk = ~(size_t)0;
    for (const gck_item_error& x : errs) chunk = std::min(chunk, (size_t)x.index / mb);
    unsigned code = 0;
    for (const gck_item_error& x : errs)
      if (x.index / mb == chunk) code = std::max(code, (unsigned)x.code);
    lookup_item_error(code);
  }
  for (size_t wd = 0; wd < plane.size(); ++wd) {
    uint64_t x = plane[wd];
    if (!x) continue;
    for (uint32_t b = 0; x; ++b, x >>= 2) {
      const uint8_t pm = (uint8_t)(x & 3u);
      if (pm != GCK_PERM_HAS && pm != GCK_PERM_CONDITIONAL) continue;
      const size_t i = wd * 32 + b;
      ids.push_back(q.ids ? q.ids[i] : q.first_id + (uint32_t)i);
      perms.push_back(pm);
    }
  }
}

// ---- LookupSubjects: the walk ------------------------------------------------------------------

struct EnumArgs {
  const unsigned long long* cur;  // this level's vertices: node << 32 | object
  uint32_t n_cur;
  unsigned long long* next;       // the next level's (first visits only)
  uint32_t next_cap;
  unsigned long long* vis;        // visited vertices, open addressing (empty = ~0)
  unsigned long long vmask;
  unsigned long long* fset;       // subjects collected, open addressing (empty = ~0)
  unsigned long long fmask;
  uint32_t* found;                // ... and as a list
  uint32_t found_cap;
  unsigned* cnt;                  // [0] next size, [1] found size, [2] overflow, [3] visited size
  uint16_t stype, srel;           // the requested subject kind
  int64_t now_us;
};

// Inserts key; true if it was not there. The callers keep the load at most 1/2 (cnt[3] / the
// found cap), so a probe sequence ends at an empty slot.
__device__ __forceinline__ bool enum_insert(unsigned long long* set, unsigned long long mask, unsigned long long key) {
  unsigned long long h = mix64(key) & mask;
  for (unsigned long long k = 0; k <= mask; ++k) {
    const unsigned long long prev = atomicCAS(&set[h], ~0ull, key);
    if (prev == ~0ull) return true;
    if (prev == key) return false;
    h = (h + 1) & mask;
  }
  return false;
}

__device__ __forceinline__ void enum_push(const EnumArgs& a, uint32_t obj, uint16_t node) {
  if (node == kNoNode) return;
  const unsigned long long key = ((unsigned long long)node << 32) | obj;
  if (!enum_insert(a.vis, a.vmask, key)) return;
  if (atomicAdd(&a.cnt[3], 1u) >= (uint32_t)((a.vmask + 1) / 2)) atomicOr(&a.cnt[2], 1u);
  const unsigned k = atomicAdd(&a.cnt[0], 1u);
  if (k < a.next_cap) a.next[k] = key;
  else atomicOr(&a.cnt[2], 2u);
}

__device__ __forceinline__ void enum_found(const EnumArgs& a, uint32_t x) {
  if (!enum_insert(a.fset, a.fmask, x)) return;
  const unsigned k = atomicAdd(&a.cnt[1], 1u);
  if (k < a.found_cap) a.found[k] = x;
  else atomicOr(&a.cnt[2], 4u);
}

// One row (object `obj` of CSR `ci`) read by the whole wave: visible neighbours x become found
// subjects when the kind is the requested one (`collect`) and vertices (x, target) otherwise.
__device__ __forceinline__ void enum_row(const Ctx& c, const EnumArgs& a, uint32_t ci, uint32_t obj, uint16_t target,
                                         bool collect, uint32_t lane) {
  if (ci == kNone) return;
  const DevCSR& r = c.csrs[ci];
  if (obj >= r.n_rows) return;
  const uint32_t b = csr_off(r, obj), en = csr_off(r, obj + 1);
  for (uint32_t p = b + lane; p < en; p += 64u) {
    const uint32_t x = csr_nbr(r, p);
    if (x == kWildcard || !visible(r, p, a.now_us)) continue;
    if (collect) enum_found(a, x);
    enum_push(a, x, target);
  }
}

// One wavefront per vertex of the level.
__global__ void __launch_bounds__(kBlock) k_enum_level(Ctx c, EnumArgs a) {
  const uint32_t v = (blockIdx.x * kBlock + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
  if (v >= a.n_cur) return;
  const unsigned long long key = a.cur[v];
  const uint32_t obj = (uint32_t)key;
  const uint16_t node = (uint16_t)(key >> 32);
  const DevNode nd = c.nodes[node];
  for (uint32_t k = 0; k < nd.count; ++k) {
    const DevItem it = c.items[nd.first + k];
    switch (nd.kind) {
      case NK_RELATION: {  // stored relationships: the requested kind is collected, usersets walked
        const bool collect = it.stype == a.stype && it.srel == a.srel;
        const uint16_t target = it.srel == kEllipsis ? kNoNode : it.target;
        if (!collect && target == kNoNode) break;
        enum_row(c, a, it.csr_plain, obj, target, collect, lane);
        enum_row(c, a, it.csr_ext, obj, target, collect, lane);
        break;
      }
      case NK_UNION:
      case NK_ARROW_ALL:
        if (it.kind == IT_ARROW) {
          enum_row(c, a, it.csr_plain, obj, it.target, false, lane);
          enum_row(c, a, it.csr_ext, obj, it.target, false, lane);
        } else if (lane == 0 && (it.kind == IT_COMPUTED || it.kind == IT_SUB)) {
          enum_push(a, obj, it.target);
        }
        break;
      case NK_INTERSECT:  // every operand can hold a subject of the result
        if (lane == 0) enum_push(a, obj, it.target);
        break;
      case NK_EXCLUDE:  // only the base can
        if (lane == 0 && k == 0) enum_push(a, obj, it.target);
        break;
      default:
        break;
    }
  }
}

__global__ void k_enum_seed(EnumArgs a, unsigned long long root) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    enum_insert(a.vis, a.vmask, root);
    a.cnt[3] = 1u;
  }
}

// A scratch device array of one call, ordered on its stream.
template <class T>
struct DeviceBuf {
  T* p = nullptr;
  hipStream_t st;
  DeviceBuf(size_t n, hipStream_t s) : st(s) {
    HIP_OK(hipMallocAsync(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T), st));
  }
  ~DeviceBuf() {
    if (p) (void)hipFreeAsync(p, st);
  }
  DeviceBuf(const DeviceBuf&) = delete;
  DeviceBuf& operator=(const DeviceBuf&) = delete;
};

// The LookupSubjects answer for proto's (resource, permission, subject kind); see the top of the
// file. Throws on a capacity no retry can meet or on a per-item error of a candidate.
void device_lookup_subjects(Engine& e, Workspace& w, const gck_item& proto, int64_t now_us, std::vector<uint32_t>& ids,
                            std::vector<uint8_t>& perms) {
  HIP_OK(hipSetDevice(e.device));
  std::lock_guard<std::mutex> lk(w.m);
  stage_caveats(w, CavCall(), w.stream);
  if (now_us == 0) now_us = wall_now_us();
  const hipStream_t st = w.stream;
  std::vector<uint32_t> cand;
  if (proto.resource_id < e.interner[proto.resource_type].count) {
    // the walk, with its tables grown (and the walk redone) until nothing overflows
    for (int scale = 0;; ++scale) {
      if (scale > 8) throw Error(GCK_E_CAPACITY, "LookupSubjects: the walk outgrows its device tables");
      const size_t vcap = (size_t)1 << (22 + scale), fcap = (size_t)1 << (20 + scale);
      DeviceBuf<unsigned long long> cur(vcap / 2, st), nxt(vcap / 2, st), vis(vcap, st), fset(2 * fcap, st);
      DeviceBuf<uint32_t> found(fcap, st);
      DeviceBuf<unsigned> cnt(4, st);
      HIP_OK(hipMemsetAsync(vis.p, 0xFF, vcap * 8, st));
      HIP_OK(hipMemsetAsync(fset.p, 0xFF, 2 * fcap * 8, st));
      HIP_OK(hipMemsetAsync(cnt.p, 0, 16, st));
      EnumArgs a{};
      a.vis = vis.p;
      a.vmask = vcap - 1;
      a.fset = fset.p;
      a.fmask = 2 * fcap - 1;
      a.found = found.p;
      a.found_cap = (uint32_t)fcap;
      a.cnt = cnt.p;
      a.stype = proto.subject_type;
      a.srel = proto.subject_relation;
      a.now_us = now_us;
      a.next_cap = (uint32_t)(vcap / 2);
      const unsigned long long root = ((unsigned long long)proto.permission << 32) | proto.resource_id;
      hipLaunchKernelGGL(k_enum_seed, dim3(1), dim3(64), 0, st, a, root);
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemcpyAsync(cur.p, &root, 8, hipMemcpyHostToDevice, st));
      Ctx c = make_ctx(e, w, now_us, st);
      unsigned h[4] = {0, 0, 0, 0};
      uint32_t n = 1;
      bool overflow = false;
      for (uint32_t level = 0; n > 0; ++level) {
        if (level > (1u << 24)) throw Error(GCK_E_DEVICE, "engine invariant violated: LookupSubjects walk does not end");
        a.cur = cur.p;
        a.n_cur = n;
        a.next = nxt.p;
        HIP_OK(hipMemsetAsync(cnt.p, 0, 4, st));  // next size
        hipLaunchKernelGGL(k_enum_level, dim3((uint32_t)(((size_t)n * 64 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                           c, a);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(h, cnt.p, 16, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (h[2]) {
          overflow = true;
          break;
        }
        n = h[0];
        std::swap(cur.p, nxt.p);
      }
      if (overflow) continue;
      cand.resize(h[1]);
      if (!cand.empty()) {
        HIP_OK(hipMemcpyAsync(cand.data(), found.p, cand.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
      }
      break;
    }
    std::sort(cand.begin(), cand.end());
  }
  // the subject no relationship names: what a wildcard grants (usersets have no wildcard)
  const bool wild = proto.subject_relation == kEllipsis;
  if (wild) cand.push_back(kAbsent);
  if (!w.lk_cnt) {  // (the same per-workspace buffers as the sweep)
    w.lk_ids = dalloc<uint32_t>(w.allocs, w.max_batch);
    w.lk_perm = dalloc<uint8_t>(w.allocs, w.max_batch);
    w.lk_cnt = dalloc<unsigned>(w.allocs, 2);
    HIP_OK(hipStreamSynchronize(nullptr));  // pool allocations are ordered on the null stream
  }
  ids.clear();
  perms.clear();
  float ms = 0.f;
  std::vector<gck_item> items;
  std::vector<uint8_t> p;
  std::vector<int32_t> er;
  for (size_t base = 0; base < cand.size(); base += w.max_batch) {
    const size_t n = std::min(cand.size() - base, w.max_batch);
    items.assign(n, proto);
    for (size_t k = 0; k < n; ++k) items[k].subject_id = cand[base + k];
    p.resize(n);
    er.resize(n);
    HIP_OK(hipMemcpyAsync(w.d_items, items.data(), n * sizeof(gck_item), hipMemcpyHostToDevice, st));
    check_range(e, w, w.d_items, n, now_us, w.d_perm, w.d_err, st, &ms);
    HIP_OK(hipMemcpyAsync(p.data(), w.d_perm, n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(er.data(), w.d_err, n * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (size_t k = 0; k < n; ++k) {
      if (er[k] != GCK_ITEM_OK)
        throw Error(GCK_E_INVALID_ARGUMENT,
                    er[k] == GCK_ITEM_ERR_MAX_DEPTH ? "max depth exceeded: this usually indicates a recursive or too "
                                                      "deep data dependency"
                                                    : "lookup failed: per-item error " + std::to_string(er[k]));
      if (p[k] != GCK_PERM_HAS && p[k] != GCK_PERM_CONDITIONAL) continue;
      ids.push_back(cand[base + k] == kAbsent ? kWildcard : cand[base + k]);
      perms.push_back(p[k]);
    }
  }
  std::lock_guard<std::mutex> sl(e.stats_mu);
  e.stats.kernel_ms = ms;
}
