// aql.inc — the join kernels dispatched straight into an HSA queue of the engine's own (included by
// engine.hip after closure.inc and labels.inc).
//
// A 64K-check batch on the closure or label join is one kernel of ~12 us on the device, but a
// hipLaunchKernel costs ~2.4 us of host time, and a batch on the engine's stream took two of them
// (the join and k_publish, which publishes the batch only after the join's end-of-kernel L2
// write-back): with 8 batches in flight the submit loop spent 5.5 us per batch in the runtime and
// the device waited for it (bench.py --trace-loop, profiles/r03s2/). Here the engine writes the
// AQL kernel-dispatch packet itself:
//
//   * the kernels come from libgck_kernels.co (the same engine.hip compiled with --genco, one
//     gfx950 code object) loaded into an HSA executable at the first snapshot;
//   * four multi-producer HSA queues per engine, the workspaces spread over them; a batch =
//     reserve a packet slot, write its kernel arguments into the workspace's kernarg block in VRAM
//     (explicit arguments plus the hidden block counts / group sizes of code object v5; written
//     through the BAR, then the HDP flushed), write the packet body, release its header, ring the
//     doorbell: ~2.3 us of host time (0.4 with the block in pinned host memory), no runtime lock;
//   * the packet carries an agent-scope acquire and a system-scope release fence and a completion
//     signal per workspace: the signal reaching 0 says the kernel has ended and its results are
//     written back past every XCD's L2, so the wait needs no k_publish, and no block needs to know
//     it is the last: each writes a summary of its counters to its own slot in host memory, which
//     the host sums after the signal (closure.inc block_summary; engine.hip aql_collect);
//   * batches in flight on different queues overlap on the device as on separate streams.
//
// Device batches on the engine's streams and host batches take this path (GCK_AQL=0 turns it off;
// a profiled batch is timed by its queue's dispatch timestamps, aql_elapsed_ms); the caller's
// streams, batches with check contexts, chained bundles and later stages launch through HIP and
// are ordered after the join by the host's wait.

// The code object and libgck.so must come from the same sources: the kernels are matched by name
// only, and a stale libgck_kernels.co beside the library (a partial rebuild, a copied install)
// would be dispatched with another Ctx / CjArgs / LjArgs layout. Both builds embed this id — the
// Makefile's hash of the engine sources (GCK_SRC_HASH) folded with the sizes of the argument
// blocks — and aql_init turns the AQL path off when the code object's differs.
#ifndef GCK_SRC_HASH
#define GCK_SRC_HASH 0x6763'6b00'0000'0000ull
#endif
constexpr uint64_t kBuildId = (uint64_t)GCK_SRC_HASH ^ ((uint64_t)sizeof(Ctx) << 40) ^ ((uint64_t)sizeof(CjArgs) << 24) ^
                              ((uint64_t)sizeof(LjArgs) << 12) ^ (uint64_t)sizeof(LjMeta) ^ ((uint64_t)sizeof(DevCSR) << 52);
}  // namespace gck
extern "C" __device__ __attribute__((used)) const uint64_t gck_kernels_build_id = gck::kBuildId;
namespace gck {

struct AqlKernel {
  uint64_t object = 0;
  uint32_t kernarg_size = 0, group = 0, priv = 0;
};

constexpr int kAqlMaxQueues = 8;
constexpr int kAqlQueues = 4;  // HSA queues per engine (aql_init)

struct AqlState {
  hsa_agent_t agent{};
  hsa_queue_t* qs[kAqlMaxQueues] = {};
  int n_queues = 1;
  std::atomic<unsigned> next_q{0};
  uint16_t fence_bits = 0;  // acquire / release fence scopes of the packet header
  hsa_executable_t exe{};
  hsa_code_object_reader_t reader{};
  bool have_exe = false, have_reader = false;
  std::string code;  // the code object (kept while the reader lives)
  std::unordered_map<std::string, AqlKernel> kernels;  // demangled name -> kernel
  std::atomic<int> queue_error{0};
  // kernarg blocks in device memory (pinned host memory when the agent has no HDP flush register): written by
  // the host through the BAR, flushed out of the host data path (HDP) before the doorbell. The
  // kernel's argument loads then read VRAM instead of crossing PCIe: config 4 at 8 in flight
  // 13.0 -> 14.7-15.1 G checks/s (2,000 steps), 9.9 -> 11.1-11.5 G (20 steps); the flush and its
  // read-back cost the submit ~1.8 us (0.5 -> 2.3 us)
  bool devargs = false;
  uint64_t tick_hz = 0;                // HSA system clock
  hsa_amd_memory_pool_t pool{};
  hsa_agent_t cpu{};
  uint32_t* hdp_flush = nullptr;
};

static hsa_status_t aql_find_cpu(hsa_agent_t agent, void* data) {
  hsa_device_type_t type;
  if (hsa_agent_get_info(agent, HSA_AGENT_INFO_DEVICE, &type) == HSA_STATUS_SUCCESS && type == HSA_DEVICE_TYPE_CPU) {
    *static_cast<hsa_agent_t*>(data) = agent;
    return HSA_STATUS_INFO_BREAK;
  }
  return HSA_STATUS_SUCCESS;
}

static hsa_status_t aql_find_pool(hsa_amd_memory_pool_t pool, void* data) {
  hsa_amd_segment_t seg;
  uint32_t flags = 0;
  bool alloc = false;
  if (hsa_amd_memory_pool_get_info(pool, HSA_AMD_MEMORY_POOL_INFO_SEGMENT, &seg) != HSA_STATUS_SUCCESS ||
      seg != HSA_AMD_SEGMENT_GLOBAL)
    return HSA_STATUS_SUCCESS;
  (void)hsa_amd_memory_pool_get_info(pool, HSA_AMD_MEMORY_POOL_INFO_GLOBAL_FLAGS, &flags);
  (void)hsa_amd_memory_pool_get_info(pool, HSA_AMD_MEMORY_POOL_INFO_RUNTIME_ALLOC_ALLOWED, &alloc);
  if (alloc && (flags & HSA_AMD_MEMORY_POOL_GLOBAL_FLAG_COARSE_GRAINED)) {
    *static_cast<hsa_amd_memory_pool_t*>(data) = pool;
    return HSA_STATUS_INFO_BREAK;
  }
  return HSA_STATUS_SUCCESS;
}

static bool aql_on() {
  // (the TIMING=1 build launches every kernel through HIP: the code object holds the product kernels)
  static const bool on = !GCK_BUNDLE_TIMING && !(getenv("GCK_AQL") && atoi(getenv("GCK_AQL")) == 0);
  return on;
}

static void aql_queue_error(hsa_status_t status, hsa_queue_t*, void* data) {
  static_cast<AqlState*>(data)->queue_error.store((int)status);
}

// the code object beside libgck.so
static std::string aql_code_path() {
  Dl_info info{};
  if (!dladdr(reinterpret_cast<void*>(&aql_code_path), &info) || !info.dli_fname) return "";
  std::string p = info.dli_fname;
  const size_t slash = p.rfind('/');
  return (slash == std::string::npos ? std::string(".") : p.substr(0, slash)) + "/libgck_kernels.co";
}

static hsa_status_t aql_find_agent(hsa_agent_t agent, void* data) {
  auto* want = static_cast<std::pair<uint32_t, hsa_agent_t*>*>(data);
  hsa_device_type_t type;
  if (hsa_agent_get_info(agent, HSA_AGENT_INFO_DEVICE, &type) != HSA_STATUS_SUCCESS || type != HSA_DEVICE_TYPE_GPU)
    return HSA_STATUS_SUCCESS;
  uint32_t bdf = 0, domain = 0;
  if (hsa_agent_get_info(agent, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf) != HSA_STATUS_SUCCESS)
    return HSA_STATUS_SUCCESS;
  (void)hsa_agent_get_info(agent, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &domain);
  if ((((uint64_t)domain << 16) | bdf) == want->first) {
    *want->second = agent;
    return HSA_STATUS_INFO_BREAK;
  }
  return HSA_STATUS_SUCCESS;
}

static hsa_status_t aql_symbol(hsa_executable_t, hsa_agent_t, hsa_executable_symbol_t sym, void* data) {
  auto* st = static_cast<AqlState*>(data);
  hsa_symbol_kind_t kind;
  if (hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_TYPE, &kind) != HSA_STATUS_SUCCESS ||
      kind != HSA_SYMBOL_KIND_KERNEL)
    return HSA_STATUS_SUCCESS;
  uint32_t len = 0;
  if (hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_NAME_LENGTH, &len) != HSA_STATUS_SUCCESS)
    return HSA_STATUS_SUCCESS;
  std::string name(len, '\0');
  if (hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_NAME, &name[0]) != HSA_STATUS_SUCCESS)
    return HSA_STATUS_SUCCESS;
  if (name.size() > 3 && name.compare(name.size() - 3, 3, ".kd") == 0) name.resize(name.size() - 3);
  int rc = 0;
  char* dm = abi::__cxa_demangle(name.c_str(), nullptr, nullptr, &rc);
  const std::string key = (rc == 0 && dm) ? std::string(dm) : name;
  std::free(dm);
  AqlKernel k;
  if (hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_OBJECT, &k.object) != HSA_STATUS_SUCCESS ||
      hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_KERNARG_SEGMENT_SIZE, &k.kernarg_size) !=
          HSA_STATUS_SUCCESS ||
      hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_GROUP_SEGMENT_SIZE, &k.group) !=
          HSA_STATUS_SUCCESS ||
      hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_PRIVATE_SEGMENT_SIZE, &k.priv) !=
          HSA_STATUS_SUCCESS)
    return HSA_STATUS_SUCCESS;
  st->kernels[key] = k;
  return HSA_STATUS_SUCCESS;
}

static void aql_free(AqlState* st) {
  if (!st) return;
  for (hsa_queue_t* q : st->qs)
    if (q) (void)hsa_queue_destroy(q);
  if (st->have_exe) (void)hsa_executable_destroy(st->exe);
  if (st->have_reader) (void)hsa_code_object_reader_destroy(st->reader);
  delete st;
  (void)hsa_shut_down();  // (reference counted: balances aql_init's hsa_init)
}

// The engine's queue and kernels, once per engine. Null when the path is off or unavailable (no
// code object beside the library, no matching agent): the batches then launch through HIP.
static AqlState* aql_init(Engine& e) {
  if (!aql_on()) return nullptr;
  std::ifstream f(aql_code_path(), std::ios::binary);
  if (!f) return nullptr;
  std::stringstream ss;
  ss << f.rdbuf();
  if (hsa_init() != HSA_STATUS_SUCCESS) return nullptr;
  auto* st = new AqlState();
  st->code = ss.str();
  int bus = 0, dev = 0, dom = 0;
  HIP_OK(hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, e.device));
  HIP_OK(hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, e.device));
  HIP_OK(hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, e.device));
  st->agent.handle = 0;
  std::pair<uint32_t, hsa_agent_t*> want{((uint32_t)dom << 16) | ((uint32_t)bus << 8) | ((uint32_t)dev << 3), &st->agent};
  (void)hsa_iterate_agents(aql_find_agent, &want);
  bool ok = st->agent.handle != 0;
  ok = ok && hsa_code_object_reader_create_from_memory(st->code.data(), st->code.size(), &st->reader) == HSA_STATUS_SUCCESS;
  st->have_reader = ok;
  ok = ok && hsa_executable_create_alt(HSA_PROFILE_FULL, HSA_DEFAULT_FLOAT_ROUNDING_MODE_DEFAULT, nullptr, &st->exe) ==
                 HSA_STATUS_SUCCESS;
  st->have_exe = ok;
  ok = ok && hsa_executable_load_agent_code_object(st->exe, st->agent, st->reader, nullptr, nullptr) == HSA_STATUS_SUCCESS;
  ok = ok && hsa_executable_freeze(st->exe, nullptr) == HSA_STATUS_SUCCESS;
  ok = ok && hsa_executable_iterate_agent_symbols(st->exe, st->agent, aql_symbol, st) == HSA_STATUS_SUCCESS;
  if (ok) {  // the code object's build id (kBuildId above) must be this library's
    hsa_executable_symbol_t sym{};
    uint64_t addr = 0, id = ~kBuildId;
    ok = hsa_executable_get_symbol_by_name(st->exe, "gck_kernels_build_id", &st->agent, &sym) == HSA_STATUS_SUCCESS &&
         hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_VARIABLE_ADDRESS, &addr) == HSA_STATUS_SUCCESS &&
         addr && hsa_memory_copy(&id, reinterpret_cast<void*>(addr), sizeof(id)) == HSA_STATUS_SUCCESS && id == kBuildId;
    if (!ok) fprintf(stderr, "[gck] libgck_kernels.co does not match libgck.so (build id): joins launch through HIP\n");
  }
  // Queues: a queue runs its dispatches one after the other (the packet processor starts the next
  // once the previous has completed, barrier bit or not), so batches overlap across queues only;
  // config 4 at 8 in flight (profiles/r03/aql/): 1 / 2 / 3 / 4 / 6 / 8 queues gave 4.5 / 9.0 /
  // 10.5 / 12.6 / 7.6 / 7.7 G checks/s, so four. Fences: the acquire invalidates the caches the
  // kernel reads through — the kernarg block of the workspace is rewritten at the same address
  // every batch, so it may not be omitted — agent scope is enough for device data; the release
  // writes the results back past every XCD's L2 at system scope, so that a host reader of a
  // zero-copy batch sees them once the completion signal is 0 (round 3 measured agent-scope
  // acquire / release, host-only completion signals and other fence scopes: none moved the
  // dispatch span or the throughput beyond run-to-run spread, DESIGN.md §10).
  st->n_queues = kAqlQueues;
  if (const char* q = debug_env("GCK_DEBUG_AQL_QUEUES"))  // (a queue-count sweep: tools/gpu.sh sweep)
    st->n_queues = std::max(1, std::min(kAqlMaxQueues, atoi(q)));
  st->fence_bits = (uint16_t)((HSA_FENCE_SCOPE_AGENT << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) |
                              (HSA_FENCE_SCOPE_SYSTEM << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE));
  // GCK_DEBUG_AQL_FENCE=<acquire>,<release> (0 none, 1 agent, 2 system): the dispatch-span
  // attribution experiment only (a scope below the default can read stale kernel arguments or
  // publish results late; not for use)
  if (const char* f = debug_env("GCK_DEBUG_AQL_FENCE")) {
    const int a = atoi(f), r = strchr(f, ',') ? atoi(strchr(f, ',') + 1) : 2;
    const int sc[3] = {HSA_FENCE_SCOPE_NONE, HSA_FENCE_SCOPE_AGENT, HSA_FENCE_SCOPE_SYSTEM};
    st->fence_bits = (uint16_t)((sc[std::min(2, std::max(0, a))] << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) |
                                (sc[std::min(2, std::max(0, r))] << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE));
  }
  const hsa_queue_type32_t qtype = debug_env("GCK_DEBUG_AQL_SINGLE") ? HSA_QUEUE_TYPE_SINGLE : HSA_QUEUE_TYPE_MULTI;
  for (int k = 0; k < st->n_queues && ok; ++k)
    ok = hsa_queue_create(st->agent, 1024, qtype, aql_queue_error, st, UINT32_MAX, UINT32_MAX,
                          &st->qs[k]) == HSA_STATUS_SUCCESS;
  if (!ok) {
    aql_free(st);
    return nullptr;
  }
  // the check batches' queues above the HIP streams: a join is latency-bound (two dependent rounds
  // of random lines), and beside a Watch build's merge kernels (config 5: ~130 MB of CSR copies per
  // batch on the null stream) its workgroups otherwise wait for CUs behind the merge's tiles
  // (the join 24 us alone, 85 us beside the merge). Best effort: a driver that refuses leaves NORMAL.
  for (int k = 0; k < st->n_queues; ++k) (void)hsa_amd_queue_set_priority(st->qs[k], HSA_AMD_QUEUE_PRIORITY_HIGH);
  // every queue records its packets' dispatch timestamps from the start (a profiled batch is
  // timed by them): enabled later, on a queue that has already run packets, the setting was not
  // always picked up — a whole process then read zero timestamps
  bool stamps = !debug_env("GCK_DEBUG_AQL_NOPROF");
  for (int k = 0; k < st->n_queues && stamps; ++k)
    stamps &= hsa_amd_profiling_set_profiler_enabled(st->qs[k], 1) == HSA_STATUS_SUCCESS;
  if (debug_env("GCK_DEBUG_AQL")) {  // where the loader put the kernels' code (device or host memory)
    for (auto& [name, k] : st->kernels) {
      if (name != cj_variant(24, true).aql_name) continue;  // (the dispatched closure join)
      hsa_amd_pointer_info_t pi{};
      pi.size = sizeof(pi);
      hsa_agent_t owner{};
      pi.agentOwner = owner;
      const hsa_status_t s = hsa_amd_pointer_info(reinterpret_cast<void*>(k.object), &pi, nullptr, nullptr, nullptr);
      hsa_device_type_t dt = HSA_DEVICE_TYPE_CPU;
      if (s == HSA_STATUS_SUCCESS && pi.agentOwner.handle) (void)hsa_agent_get_info(pi.agentOwner, HSA_AGENT_INFO_DEVICE, &dt);
      fprintf(stderr, "[gck aql] %s object=%p info=%d type=%d owner=%s host=%p bytes=%zu\n", name.c_str(),
              (void*)k.object, (int)s, (int)pi.type, dt == HSA_DEVICE_TYPE_GPU ? "gpu" : "cpu", pi.hostBaseAddress,
              pi.sizeInBytes);
    }
  }
  (void)hsa_system_get_info(HSA_SYSTEM_INFO_TIMESTAMP_FREQUENCY, &st->tick_hz);
  if (!stamps) st->tick_hz = 0;  // (no timestamps: profiled batches launch through HIP, engine.hip)
  {
    hsa_amd_hdp_flush_t hdp{};
    st->pool.handle = 0;
    st->cpu.handle = 0;
    if (hsa_agent_get_info(st->agent, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_HDP_FLUSH, &hdp) == HSA_STATUS_SUCCESS &&
        hdp.HDP_MEM_FLUSH_CNTL) {
      (void)hsa_iterate_agents(aql_find_cpu, &st->cpu);
      (void)hsa_amd_agent_iterate_memory_pools(st->agent, aql_find_pool, &st->pool);
      st->hdp_flush = hdp.HDP_MEM_FLUSH_CNTL;
      st->devargs = st->cpu.handle && st->pool.handle;
      if (debug_env("GCK_DEBUG_AQL_HOSTARGS")) st->devargs = false;  // (the attribution experiment)
    }
  }
  return st;
}

static const AqlKernel* aql_kernel(const AqlState* st, const char* name) {
  auto it = st->kernels.find(name);
  return it == st->kernels.end() ? nullptr : &it->second;
}

// Per workspace: the kernarg block (pinned, coherent: the kernel reads its arguments from it) and
// the completion signal.
constexpr size_t kAqlKernargBytes = 1024;
// ... whose upper half holds what a dispatched kernel reads through a pointer argument (the
// label join's Ctx of a batch with check contexts): written with the arguments, no copy on a stream
constexpr size_t kAqlExtraOff = 512;
static_assert(sizeof(Ctx) <= kAqlKernargBytes - kAqlExtraOff, "a batch's Ctx fits the kernarg block");

// The device address of the block's extra region (aql_dispatch `extra`).
static const void* aql_extra(const Workspace& w) { return static_cast<const unsigned char*>(w.aql_kernarg) + kAqlExtraOff; }

// Host writes into VRAM through the BAR are complete once the HDP has been flushed (a register
// write, read back).
static void aql_hdp_flush(const AqlState& st) {
  __builtin_ia32_sfence();
  *reinterpret_cast<volatile uint32_t*>(st.hdp_flush) = 1u;
  (void)*reinterpret_cast<volatile uint32_t*>(st.hdp_flush);
}

// The extra region written alone, for a kernel launched through HIP that reads it (the label join's
// Ctx on the engine's stream: no copy before it on the stream). The workspace runs one batch at a
// time, so no kernel still reads the region's previous contents.
static void aql_put_extra(const AqlState& st, Workspace& w, const void* extra, size_t bytes) {
  auto* dst = static_cast<unsigned char*>(w.aql_kernarg) + kAqlExtraOff;
  const auto* src = static_cast<const unsigned char*>(extra);
  for (size_t o = 0; o < bytes; o += 16) {
    const size_t n = std::min<size_t>(16, bytes - o);
    if (std::memcmp(src + o, w.aql_shadow + kAqlExtraOff + o, n) == 0) continue;
    std::memcpy(dst + o, src + o, n);
    std::memcpy(w.aql_shadow + kAqlExtraOff + o, src + o, n);
  }
  aql_hdp_flush(st);
}

// A shaped batch's table (closure.inc CjArgs::shapes) in the workspace's own block behind the
// kernarg block — the same memory, written the same way: only the 16-B entries that differ from
// what it holds (a caller's requests mostly repeat one table), then the HDP flush. The workspace
// runs one batch at a time, so no kernel still reads the previous table.
constexpr size_t kAqlShapesBytes = GCK_MAX_SHAPES * sizeof(gck_uniform);
static_assert(sizeof(gck_uniform) == 16, "a shape is one 16-B entry");
static void aql_put_shapes(const AqlState& st, Workspace& w, const gck_uniform* shapes, uint32_t n_shapes) {
  static_assert(sizeof(w.shapes_shadow) == kAqlShapesBytes, "shape table shadow size");
  auto* dst = static_cast<unsigned char*>(w.aql_shapes);
  const auto* src = reinterpret_cast<const unsigned char*>(shapes);
  bool wrote = false;
  for (size_t o = 0; o < (size_t)n_shapes * 16; o += 16) {
    if (std::memcmp(src + o, w.shapes_shadow + o, 16) == 0) continue;
    std::memcpy(dst + o, src + o, 16);
    std::memcpy(w.shapes_shadow + o, src + o, 16);
    wrote = true;
  }
  if (wrote && w.aql_devargs) aql_hdp_flush(st);
}

// A cross batch's id block (closure.inc CjArgs::cols) behind the shape-table block, in the same
// allocation and written the same way: the tile's resource ids, then its subject ids from word
// cross_sub_off(cols); only the 16-B lines that differ from what the block holds — a tile that
// moves along a row band rewrites the resource ids alone, a caller paging through resources for
// one subject likewise — then one HDP flush. GCK_CROSS_IDS ids and the 12 B the subjects' alignment
// can take.
constexpr size_t kAqlIdsBytes = (size_t)GCK_CROSS_IDS * 4 + 16;
static void aql_put_ids(const AqlState& st, Workspace& w, const uint32_t* resources, uint32_t cols, const uint32_t* subjects,
                        uint32_t rows) {
  static_assert(sizeof(w.ids_shadow) == kAqlIdsBytes, "id block shadow size");
  const size_t sub = (size_t)cross_sub_off(cols) * 4, end = sub + (size_t)rows * 4;
  if (end > kAqlIdsBytes) throw Error(GCK_E_DEVICE, "engine invariant violated: cross tile beyond the id block");
  auto* dst = static_cast<unsigned char*>(w.aql_ids);
  bool wrote = false;
  // (each list begins a 16-B line; the words between the resource ids' end and `sub` are never read)
  auto put = [&](size_t at, const uint32_t* ids, size_t len) {
    const auto* src = reinterpret_cast<const unsigned char*>(ids);
    for (size_t o = 0; o < len; o += 16) {
      const size_t n = std::min<size_t>(16, len - o);
      if (std::memcmp(src + o, w.ids_shadow + at + o, n) == 0) continue;
      std::memcpy(dst + at + o, src + o, n);
      std::memcpy(w.ids_shadow + at + o, src + o, n);
      wrote = true;
    }
  };
  put(0, resources, (size_t)cols * 4);
  put(sub, subjects, (size_t)rows * 4);
  if (wrote && w.aql_devargs) aql_hdp_flush(st);
}

constexpr size_t kAqlBlockBytes = kAqlKernargBytes + kAqlShapesBytes + kAqlIdsBytes;
static bool aql_workspace(AqlState& st, Workspace& w) {
  if (w.aql_kernarg) return true;
  void* p = nullptr;
  if (st.devargs) {  // a VRAM block the host may write (zeroed: a kernel reading it does nothing)
    if (hsa_amd_memory_pool_allocate(st.pool, kAqlBlockBytes, 0, &p) == HSA_STATUS_SUCCESS) {
      if (hsa_amd_agents_allow_access(1, &st.cpu, nullptr, p) == HSA_STATUS_SUCCESS) {
        std::memset(p, 0, kAqlBlockBytes);
        aql_hdp_flush(st);
        w.aql_devargs = true;
      } else {
        (void)hsa_amd_memory_pool_free(p);
        p = nullptr;
      }
    }
  }
  if (!p) {  // (no HDP flush register: pinned host memory, zeroed as the VRAM block is)
    if (hipHostMalloc(&p, kAqlBlockBytes, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) return false;
    std::memset(p, 0, kAqlBlockBytes);
  }
  hsa_signal_t s;
  // (GCK_DEBUG_AQL_SIGNAL: a signal without the completion interrupt — the host only spins on it —
  // for the dispatch-span attribution, tools/aql_span.sh)
  const hsa_status_t sc = debug_env("GCK_DEBUG_AQL_SIGNAL")
                              ? hsa_amd_signal_create(0, 0, nullptr, HSA_AMD_SIGNAL_AMD_GPU_ONLY, &s)
                              : hsa_signal_create(0, 0, nullptr, &s);
  if (sc != HSA_STATUS_SUCCESS) {
    if (w.aql_devargs) (void)hsa_amd_memory_pool_free(p);
    else (void)hipHostFree(p);
    w.aql_devargs = false;
    return false;
  }
  w.aql_kernarg = p;
  w.aql_shapes = static_cast<unsigned char*>(p) + kAqlKernargBytes;
  std::memset(w.shapes_shadow, 0, sizeof(w.shapes_shadow));
  w.aql_ids = static_cast<unsigned char*>(p) + kAqlKernargBytes + kAqlShapesBytes;
  std::memset(w.ids_shadow, 0, sizeof(w.ids_shadow));
  w.aql_signal = s.handle;
  return true;
}

static void aql_workspace_free(Workspace& w) {
  if (w.aql_signal) {
    hsa_signal_t s{w.aql_signal};
    (void)hsa_signal_destroy(s);
    w.aql_signal = 0;
  }
  if (w.aql_kernarg && w.aql_devargs) (void)hsa_amd_memory_pool_free(w.aql_kernarg);
  else if (w.aql_kernarg) (void)hipHostFree(w.aql_kernarg);
  w.aql_kernarg = nullptr;
  w.aql_shapes = nullptr;
  w.aql_ids = nullptr;
  w.aql_devargs = false;
  w.aql_queue = nullptr;
}

// One kernel over `blocks` blocks of kBlock threads: the explicit arguments (args, bytes: the
// kernel's by-value parameters laid out as its kernarg segment has them), then the code object
// v5 hidden arguments the kernels read (block counts, group sizes, grid dimensions).
static void aql_dispatch(AqlState& st, Workspace& w, const AqlKernel& k, const void* args, size_t bytes,
                         uint32_t blocks, bool timed = false, const void* extra = nullptr, size_t extra_bytes = 0) {
  const size_t hid = (bytes + 7) & ~(size_t)7;
  // the explicit arguments, then the whole code-object-v5 hidden block (256 B)
  if (hid + 256 != k.kernarg_size || k.kernarg_size > (extra ? kAqlExtraOff : kAqlKernargBytes) ||
      extra_bytes > kAqlKernargBytes - kAqlExtraOff)
    throw Error(GCK_E_DEVICE, "engine invariant violated: kernarg layout of a dispatched kernel");
  alignas(16) unsigned char img[kAqlKernargBytes];
  std::memset(img, 0, hid + 256);
  std::memcpy(img, args, bytes);
  const uint32_t bc[3] = {blocks, 1u, 1u};
  const uint16_t gs[3] = {(uint16_t)kBlock, 1u, 1u};
  const uint16_t dims = 1;
  std::memcpy(img + hid + 0, bc, sizeof(bc));   // hidden_block_count_x/y/z
  std::memcpy(img + hid + 12, gs, sizeof(gs));  // hidden_group_size_x/y/z (remainders 0)
  std::memcpy(img + hid + 64, &dims, 2);        // hidden_grid_dims
  // (the rest of the hidden block is zero)
  // Only the 16-byte lines that differ from what the block already holds are written: a batch
  // changes a few pointers and its size, and each line written through the BAR costs the submit.
  static_assert(sizeof(w.aql_shadow) == kAqlKernargBytes, "kernarg shadow size");
  auto* dst = static_cast<unsigned char*>(w.aql_kernarg);
  auto put = [&](size_t at, const unsigned char* src, size_t len) {
    for (size_t o = 0; o < len; o += 16) {
      const size_t n = std::min<size_t>(16, len - o);
      if (std::memcmp(src + o, w.aql_shadow + at + o, n) == 0) continue;
      std::memcpy(dst + at + o, src + o, n);
      std::memcpy(w.aql_shadow + at + o, src + o, n);
    }
  };
  put(0, img, hid + 256);
  if (extra) put(kAqlExtraOff, static_cast<const unsigned char*>(extra), extra_bytes);
  if (w.aql_devargs) aql_hdp_flush(st);
  hsa_signal_t sig{w.aql_signal};
  hsa_signal_store_relaxed(sig, 1);
  if (!w.aql_queue) w.aql_queue = st.qs[st.next_q.fetch_add(1) % (unsigned)st.n_queues];
  hsa_queue_t* q = static_cast<hsa_queue_t*>(w.aql_queue);
  const uint64_t idx = hsa_queue_add_write_index_screlease(q, 1);
  while (idx - hsa_queue_load_read_index_scacquire(q) >= q->size) __builtin_ia32_pause();
  auto* p = static_cast<hsa_kernel_dispatch_packet_t*>(q->base_address) + (idx & (q->size - 1));
  p->workgroup_size_x = (uint16_t)kBlock;
  p->workgroup_size_y = 1;
  p->workgroup_size_z = 1;
  p->reserved0 = 0;
  p->grid_size_x = blocks * kBlock;
  p->grid_size_y = 1;
  p->grid_size_z = 1;
  p->private_segment_size = k.priv;
  p->group_segment_size = k.group;
  p->kernel_object = k.object;
  p->kernarg_address = w.aql_kernarg;
  p->reserved2 = 0;
  p->completion_signal = sig;
  const uint16_t header = (uint16_t)((HSA_PACKET_TYPE_KERNEL_DISPATCH << HSA_PACKET_HEADER_TYPE) | st.fence_bits);
  const uint16_t setup = 1u << HSA_KERNEL_DISPATCH_PACKET_SETUP_DIMENSIONS;
  __atomic_store_n(reinterpret_cast<uint32_t*>(p), (uint32_t)header | ((uint32_t)setup << 16), __ATOMIC_RELEASE);
  hsa_signal_store_screlease(q->doorbell_signal, (hsa_signal_value_t)idx);
  static const bool dbg = debug_env("GCK_DEBUG_AQL") != nullptr;
  static std::atomic<int> n_dbg{0};
  if (dbg && n_dbg.fetch_add(1) < 8)
    fprintf(stderr, "[gck aql] dispatch queue=%p id=%lu idx=%lu size=%u read=%lu kernarg=%p devargs=%d\n", (void*)q,
            (unsigned long)q->id,
            (unsigned long)idx, q->size, (unsigned long)hsa_queue_load_read_index_relaxed(q), w.aql_kernarg,
            (int)w.aql_devargs);
}

// Spins until the batch's kernel has ended (its completion signal is 0). A queue error or a
// kernel that runs for 30 s ends the wait with an error instead.
// GCK_DEBUG_AQL=1: a wait still spinning after 2 s reports its signal and its queue's indices on
// stderr once a second (diagnosis of a stalled dispatch, e.g. under a profiler's queue interception)
static void aql_wait(AqlState& st, Workspace& w) {
  hsa_signal_t sig{w.aql_signal};
  static const bool dbg = debug_env("GCK_DEBUG_AQL") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  int reported = 1;
  for (uint64_t it = 1; hsa_signal_load_scacquire(sig) != 0; ++it) {
    if ((it & 4095) == 0) {
      if (st.queue_error.load()) throw Error(GCK_E_DEVICE, "HSA queue error in a dispatched join");
      const auto dt = std::chrono::steady_clock::now() - t0;
      if (dbg && dt > std::chrono::seconds(reported + 1)) {
        ++reported;
        hsa_queue_t* q = static_cast<hsa_queue_t*>(w.aql_queue);
        fprintf(stderr, "[gck aql] wait %ds: signal=%ld queue=%p id=%lu read=%lu write=%lu doorbell=%lu\n", reported,
                (long)hsa_signal_load_relaxed(sig), (void*)q, q ? (unsigned long)q->id : 0ul,
                q ? (unsigned long)hsa_queue_load_read_index_relaxed(q) : 0ul,
                q ? (unsigned long)hsa_queue_load_write_index_relaxed(q) : 0ul,
                q ? (unsigned long)q->doorbell_signal.handle : 0ul);
      }
      if (dt > std::chrono::seconds(30)) throw Error(GCK_E_DEVICE, "a dispatched join did not finish in 30 s");
    }
    __builtin_ia32_pause();
  }
}

// Waits for every dispatched join still running (before the snapshot or the workspaces go).
static void aql_drain(Engine& e) {
  if (!e.aql) return;
  for (Workspace* w : e.ws_pool)
    if (w->aql_signal) {
      hsa_signal_t sig{w->aql_signal};
      (void)hsa_signal_wait_scacquire(sig, HSA_SIGNAL_CONDITION_EQ, 0, UINT64_MAX, HSA_WAIT_STATE_ACTIVE);
    }
}

// The device time of a finished dispatched batch (GCK_FLAG_PROFILE): from its packet's processing
// start to its completion, the timestamps the queue records (the same span a profiler's kernel
// trace reports); 0 when the queue had none.
static float aql_elapsed_ms(const AqlState& st, const Workspace& w) {
  hsa_amd_profiling_dispatch_time_t t{};
  hsa_signal_t sig{w.aql_signal};
  if (!st.tick_hz || hsa_amd_profiling_get_dispatch_time(st.agent, sig, &t) != HSA_STATUS_SUCCESS || t.end <= t.start)
    return 0.f;
  return (float)((double)(t.end - t.start) * 1e3 / (double)st.tick_hz);
}
