// resident.inc — the resident closure join (included by engine.hip after aql.inc).
//
// A request of 8,192 checks (a 64K request over 8 GPUs) is one dispatch of ~64 blocks: it spends
// most of its ~10 us in the packet processor, the launch ramp and the completion, and a queue runs
// its dispatches one after another, so four queues sustain ~2.9 G checks/s where 64K-check
// dispatches sustain 11-17 G (DESIGN.md §4, profiles/r05/scaling/). The resident join takes the
// dispatch out of the request: one long-running launch per engine (gck_config.flags
// GCK_FLAG_RESIDENT) whose workgroups take 128-check chunks of the requests the host posts.
//
//   host (res_post): the request's join arguments (CjArgs, the workspace's counters, its
//     completion word and sequence) into the workspace's slot of a pinned-host table, a ring entry
//     {slot, first chunk, chunks, post}, then the post count — plain stores to coherent pinned
//     memory, no runtime call, no doorbell;
//   poller (block 0, one wave): polls the post count over PCIe (one wave, s_sleep between polls),
//     copies each new post's entry and arguments into device memory with write-through (sc1)
//     stores, drains them (vmcnt 0), then publishes the chunk total (an sc1 store);
//   workers (the other blocks, 3 per CU): claim chunk k = atomicAdd(next, 1) (the next claim taken
//     while the current chunk runs); wait (sc1 polls)
//     until k is published; find k's post from their cursor (never behind `base`, the oldest post
//     with unclaimed chunks, so no ring entry they read has been reused); an agent-scope acquire when
//     the chunk belongs to a post the block has not worked on yet (the request's items and the
//     caller's buffers were written before the post, by kernels or copies that ended with a
//     release); cj_block over the chunk; every wave's stores drained and a system-scope release;
//     then the post's finished count — the last chunk resets it and writes the sequence into the
//     workspace's completion word in host memory, which the host's wait polls.
//
// Exit: the host seals an instance (res_seal: a sealed word after its last post) before anything
// the instance read changes — a snapshot commit or Watch publication, engine teardown — and when it
// has been idle for kResIdleSeal; the poller then publishes the seal and every worker leaves once
// the chunks before it are claimed. Each wait on the device also ends after kResHardTicks
// (2 s of no progress), marking the instance dead (the host then fails the requests still posted
// to it with GCK_E_DEVICE instead of waiting): no wave of the grid can outlive its process.

constexpr uint32_t kResRing = 256;    // ring entries: posts in flight stay far below (one per workspace)
constexpr uint32_t kResSlots = 64;    // workspaces (a workspace runs one request at a time)
// worker blocks per CU: 2 of the 3 its register count allows, so that the kernels a request's
// wait launches after it (the bundles of its deferred checks, other streams' work) find room beside
// the workers that poll for the next post — with 3 they could not be scheduled, the host posted
// nothing while it waited for them, and the workers' publication wait ended the instance (2 s)
constexpr uint32_t kResPerCu = 2;
constexpr unsigned long long kResHardTicks = 200000000ull;  // 2 s at wall_clock64's 100 MHz

struct ResPost {      // one request in the ring
  uint32_t slot;      // its workspace's slot
  uint32_t start;     // its first chunk (chunks are numbered across posts)
  uint32_t n_chunks;
  uint32_t post;      // its post number
};
struct alignas(16) ResArgs {  // a slot: the request's join arguments and completion
  CjArgs a;
  DevCounters* ctr;
  unsigned* done;     // device address of the slot's completion word (ResHost::done)
  uint32_t seq;       // written to *done by the last chunk
};
static_assert(sizeof(ResArgs) % 16 == 0, "slot copies move 16-B chunks");
struct ResHost {      // pinned host memory (coherent: never cached on the device)
  uint32_t posted;    // posts published (the host's release store)
  uint32_t sealed;    // 1: no post after `posted`
  uint32_t dead;      // the device gave up (a wait passed kResHardTicks)
  uint32_t consumed;  // posts the poller has copied
  uint32_t why[4];    // the device's reason for `dead` (kResWhy*) and three values it saw, for the host's error
  uint32_t pad[8];
  ResPost ring[kResRing];
  ResArgs slots[kResSlots];
  uint32_t done[kResSlots][16];  // per slot, a line of its own: the sequence of its last finished request
};
struct ResDev {       // device memory
  unsigned long long pub;  // chunks published | sealed << 32 (sc1 stores and loads)
  unsigned next;           // chunks claimed
  unsigned base;           // the oldest post with unclaimed chunks
  unsigned finished[kResSlots];
  ResPost ring[kResRing];
  ResArgs slots[kResSlots];
};

__device__ __forceinline__ unsigned long long res_ld64(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (global_load sc1)
}
__device__ __forceinline__ uint32_t res_ld32(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t res_ld_host(const uint32_t* p) {  // pinned host memory
  return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// Why an instance died (ResHost::why[0]): a torn ring entry, an idle poller, a worker's wait for
// publication past kResHardTicks, a claimed chunk no ring entry holds.
enum : uint32_t { kResWhyTorn = 1, kResWhyIdle = 2, kResWhyPub = 3, kResWhyRing = 4 };
__device__ __forceinline__ void res_die(ResHost* h, uint32_t why, uint32_t x, uint32_t y, uint32_t z) {
  __hip_atomic_store(&h->why[1], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&h->why[2], y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&h->why[3], z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&h->why[0], why, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&h->dead, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The poller: one wave. Copies new posts into device memory and publishes their chunks.
__device__ void res_poll(ResDev* d, ResHost* h) {
  const int lane = threadIdx.x & 63;
  uint32_t seen = 0, total = 0;
  unsigned long long idle0 = wall_clock64();
  for (;;) {
    const uint32_t sealed = res_ld_host(&h->sealed);
    const uint32_t posted = res_ld_host(&h->posted);
    const bool changed = seen != posted;
    bool bad = false;
    for (; seen < posted && !bad; ++seen) {
      const ResPost e = h->ring[seen % kResRing];
      bad = e.post != seen || e.start != total || e.slot >= kResSlots || e.n_chunks == 0;
      if (bad) break;
      // the slot's arguments: 16 B per lane, write-through
      constexpr uint32_t kChunks = sizeof(ResArgs) / 16;
      if ((uint32_t)lane < kChunks) {
        const u32x4 v = *reinterpret_cast<const volatile u32x4*>(reinterpret_cast<const unsigned char*>(&h->slots[e.slot]) +
                                                                 16u * lane);
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(&d->slots[e.slot]) + 2 * lane;
        __hip_atomic_store(dst, (unsigned long long)v.x | ((unsigned long long)v.y << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(dst + 1, (unsigned long long)v.z | ((unsigned long long)v.w << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
      if (lane == 0) {
        unsigned long long* r = reinterpret_cast<unsigned long long*>(&d->ring[seen % kResRing]);
        __hip_atomic_store(r, (unsigned long long)e.slot | ((unsigned long long)e.start << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(r + 1, (unsigned long long)e.n_chunks | ((unsigned long long)e.post << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
      total += e.n_chunks;
    }
    if (bad) {  // a torn or out-of-order entry: give up (the host fails what it posted)
      if (lane == 0) {
        res_die(h, kResWhyTorn, seen, total, posted);
        __hip_atomic_store(&d->pub, (unsigned long long)total | (1ull << 32), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      }
      return;
    }
    const bool fin = sealed && seen == posted;
    if (changed || fin) {
      __builtin_amdgcn_s_waitcnt(0);  // (the copies' write-through stores have completed)
      if (lane == 0) {
        __hip_atomic_store(&d->pub, (unsigned long long)total | (fin ? 1ull << 32 : 0ull), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&h->consumed, seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
    if (fin) return;
    if (seen == posted) {
      if (wall_clock64() - idle0 > kResHardTicks) {  // no post for 2 s: retire (the host seals long before)
        if (lane == 0) {
          res_die(h, kResWhyIdle, seen, total, posted);
          __hip_atomic_store(&d->pub, (unsigned long long)total | (1ull << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return;
      }
      __builtin_amdgcn_s_sleep(4);
    } else {
      idle0 = wall_clock64();
    }
  }
}

template <int BITS, uint32_t TAB, uint32_t CPW, bool HALF>
__global__ void __launch_bounds__(kBlock) k_cj_resident(ResDev* d, ResHost* h, const unsigned char* table,
                                                        uint32_t table_bytes) {
  if (blockIdx.x == 0) {
    if (threadIdx.x < 64) res_poll(d, h);
    return;
  }
  __shared__ uint32_t s_claim[5];  // slot, chunk, chunks, post, exit
  uint32_t cur = 0;                // (thread 0) the post cursor
  uint32_t last_post = 0xFFFFFFFFu;
  bool first = true;
  // (thread 0) the next claim, taken while the block works on the current chunk: the atomic's
  // round trip overlaps the join (its wait for publication stays at the top of the loop, so a
  // request's last chunk never waits for a later post)
  uint32_t k_next = 0, b_next = 0;
  if (threadIdx.x == 0) {
    b_next = res_ld32(&d->base);
    k_next = atomicAdd(&d->next, 1u);
  }
  for (;;) {
    if (threadIdx.x == 0) {
      const uint32_t b0 = b_next;
      const uint32_t k = k_next;
      const unsigned long long t0 = wall_clock64();
      uint32_t ex = 0;
      for (;;) {
        const unsigned long long pub = res_ld64(&d->pub);
        if (k < (uint32_t)pub) break;
        if (pub >> 32) {
          ex = 1;
          break;
        }
        if (wall_clock64() - t0 > kResHardTicks) {
          res_die(h, kResWhyPub, k, (uint32_t)pub, blockIdx.x);
          ex = 1;
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
      if (!ex) {
        cur = max(cur, b0);
        for (uint32_t guard = 0;; ++guard) {
          const unsigned long long* r = reinterpret_cast<const unsigned long long*>(&d->ring[cur % kResRing]);
          const unsigned long long x0 = res_ld64(r), x1 = res_ld64(r + 1);
          const uint32_t start = (uint32_t)(x0 >> 32), n = (uint32_t)x1, post = (uint32_t)(x1 >> 32);
          if (post != cur || guard > kResRing) {  // (cannot happen: k is published, so is its post)
            res_die(h, kResWhyRing, k, cur, post);
            ex = 1;
            break;
          }
          if (k - start < n) {
            if (k - start == n - 1u) atomicMax(&d->base, cur + 1u);  // (its last chunk is claimed)
            s_claim[0] = (uint32_t)x0;
            s_claim[1] = k - start;
            s_claim[2] = n;
            s_claim[3] = cur;
            break;
          }
          ++cur;
        }
      }
      s_claim[4] = ex;
    }
    __syncthreads();
    if (s_claim[4]) break;
    if (threadIdx.x == 0) {
      b_next = res_ld32(&d->base);
      k_next = atomicAdd(&d->next, 1u);
    }
    const uint32_t slot = __builtin_amdgcn_readfirstlane(s_claim[0]);
    const uint32_t chunk = __builtin_amdgcn_readfirstlane(s_claim[1]);
    const uint32_t n_chunks = __builtin_amdgcn_readfirstlane(s_claim[2]);
    const uint32_t post = __builtin_amdgcn_readfirstlane(s_claim[3]);
    if (post != last_post) {
      // a request this block has not worked on: what its caller wrote before the post (items,
      // pairs) and the slot's arguments are read after an agent-scope acquire
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      last_post = post;
    }
    // the slot's arguments (write-through copies: sc1 loads), uniform across the block (held in
    // scalar registers: the kernel takes 134 VGPRs: 3 blocks per CU would fit, kResPerCu)
    ResArgs ra;
    {
      const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&d->slots[slot]);
      unsigned long long tmp[sizeof(ResArgs) / 8];
#pragma unroll
      for (uint32_t q = 0; q < sizeof(ResArgs) / 8; ++q) {
        const unsigned long long v = res_ld64(src + q);
        tmp[q] = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
                 (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
      }
      __builtin_memcpy(&ra, tmp, sizeof(ResArgs));
    }
    // results written through the L2 (sc1 stores: their readers are other kernels and the host, and
    // this launch never ends to write its L2 back); the snapshot's table staged once per launch
    CjArgs a = ra.a;
    a.table = table;
    a.table_bytes = table_bytes;
    a.mode |= kPubCoherent;
    const CjLocalArgs ax{cj_hot(a), &a, ra.ctr, n_chunks};
    const uint32_t deferred = cj_block<BITS, TAB, CPW, HALF>(
        ax, chunk, first, (GCK_BUNDLE_TIMING && (a.mode & kCjTimed)) ? wall_clock64() : 0ull);
    first = false;
    // every wave's stores have completed, then the chunk counts towards its request
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (threadIdx.x == 0) {
      // the deferred list and the items written for the bundle stages are plain stores: written
      // back (agent scope) when the chunk left any
      if (deferred) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      const uint32_t f = atomicAdd(&d->finished[slot], 1u);
      if (f + 1u == n_chunks) {
        __hip_atomic_store(&d->finished[slot], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ra.done, ra.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

// (dispatched by name from libgck_kernels.co, never launched through HIP: instantiated here)
template __global__ void k_cj_resident<24, kCjLdsBytesSmall, 32, true>(ResDev*, ResHost*, const unsigned char*, uint32_t);

// ---- host side --------------------------------------------------------------------------------
constexpr uint32_t kResMaxChunks = 1u << 30;  // a launch is sealed before its chunk numbers wrap
constexpr int kResIdleSealMs = 20;             // an idle launch is sealed after this (keeper thread)
constexpr const char* kResKernel =
    "void gck::k_cj_resident<24, 2048u, 32u, true>(gck::ResDev*, gck::ResHost*, unsigned char const*, unsigned int)";

struct ResState {
  ResHost* h = nullptr;      // pinned, coherent
  ResHost* h_dev = nullptr;  // its device address
  ResDev* d = nullptr;
  hsa_queue_t* q = nullptr;
  hsa_signal_t sig{};
  void* kernarg = nullptr;   // pinned
  const AqlKernel* k = nullptr;
  uint32_t blocks = 0;
  std::mutex mu;             // posts, launches, seals
  bool running = false;
  uint32_t posts = 0, chunks = 0, inflight = 0;
  uint32_t seq_posted[kResSlots] = {};  // per slot, the sequence of its last post (device-done: done == it)
  const void* table = nullptr;
  uint32_t table_bytes = 0;
  std::chrono::steady_clock::time_point last;
  std::thread keeper;
  std::atomic<bool> stop{false};
  uint64_t launches = 0;
  hipStream_t st = nullptr;  // (the control block's reset before a launch)
};

// Every posted request's last chunk has finished on the device (its caller may not have waited yet).
static bool res_device_idle(const ResState& r) {
  for (uint32_t s = 0; s < kResSlots; ++s)
    if (__atomic_load_n(&r.h->done[s][0], __ATOMIC_ACQUIRE) != r.seq_posted[s]) return false;
  return true;
}

// Seals the running launch and waits for its grid to drain (caller holds r.mu; every posted request
// finished on the device, res_device_idle).
static void res_seal_locked(ResState& r) {
  if (!r.running) return;
  __atomic_store_n(&r.h->sealed, 1u, __ATOMIC_RELEASE);
  const auto t0 = std::chrono::steady_clock::now();
  while (hsa_signal_wait_scacquire(r.sig, HSA_SIGNAL_CONDITION_EQ, 0, 1000000, HSA_WAIT_STATE_ACTIVE) != 0) {
    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) {
      r.running = false;  // (its waves leave on their own time limit)
      throw Error(GCK_E_DEVICE, "the resident join did not drain after its seal");
    }
  }
  r.running = false;
}

static void res_keeper(Engine* e) {
  ResState& r = *e->res;
  while (!r.stop.load()) {
    std::this_thread::sleep_for(std::chrono::milliseconds(1));
    std::lock_guard<std::mutex> lk(r.mu);
    // idle: nothing in flight for kResIdleSealMs, or requests in flight whose device work has all
    // finished and no post for 1 ms (their callers are busy elsewhere: the workers go, and give
    // their CUs back, until the next post launches again)
    const auto idle = std::chrono::steady_clock::now() - r.last;
    if (r.running && ((r.inflight == 0 && idle > std::chrono::milliseconds(kResIdleSealMs)) ||
                      (idle > std::chrono::milliseconds(1) && res_device_idle(r)))) {
      try {
        res_seal_locked(r);
      } catch (const Error&) {
      }
    }
  }
}

// The engine's resident join, when gck_config.flags has GCK_FLAG_RESIDENT and the code object is
// loaded (the AQL path); null otherwise (batches take their own dispatch).
static ResState* res_init(Engine& e) {
  if (!(e.cfg.flags & GCK_FLAG_RESIDENT) || !e.aql) return nullptr;
  const AqlKernel* k = aql_kernel(e.aql, kResKernel);
  if (!k) return nullptr;
  auto* r = new ResState();
  r->k = k;
  HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&r->h), sizeof(ResHost), hipHostMallocCoherent | hipHostMallocMapped));
  std::memset(r->h, 0, sizeof(ResHost));
  HIP_OK(hipHostGetDevicePointer(reinterpret_cast<void**>(&r->h_dev), r->h, 0));
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&r->d), sizeof(ResDev)));
  HIP_OK(hipHostMalloc(&r->kernarg, 512, hipHostMallocCoherent | hipHostMallocMapped));
  HIP_OK(hipStreamCreateWithFlags(&r->st, hipStreamNonBlocking));
  bool ok = hsa_queue_create(e.aql->agent, 64, HSA_QUEUE_TYPE_MULTI, aql_queue_error, e.aql, UINT32_MAX, UINT32_MAX,
                             &r->q) == HSA_STATUS_SUCCESS;
  ok = ok && hsa_signal_create(0, 0, nullptr, &r->sig) == HSA_STATUS_SUCCESS;
  if (!ok) {
    if (r->q) (void)hsa_queue_destroy(r->q);
    (void)hipHostFree(r->h);
    (void)hipHostFree(r->kernarg);
    (void)hipFree(r->d);
    (void)hipStreamDestroy(r->st);
    delete r;
    return nullptr;
  }
  r->blocks = 1 + device_cus(e.device) * kResPerCu;
  r->last = std::chrono::steady_clock::now();
  return r;
}

static void res_start_keeper(Engine& e) {
  if (e.res && !e.res->keeper.joinable()) e.res->keeper = std::thread(res_keeper, &e);
}

// A new launch over `table` (caller holds r.mu; nothing of the previous launch in flight).
static void res_launch(Engine& e, ResState& r, const void* table, uint32_t table_bytes) {
  HIP_OK(hipMemsetAsync(r.d, 0, offsetof(ResDev, ring), r.st));
  HIP_OK(hipStreamSynchronize(r.st));
  r.h->posted = r.h->sealed = r.h->dead = r.h->consumed = 0;
  std::memset(r.h->why, 0, sizeof(r.h->why));
  // (the completion words keep their sequences: a request finished under the previous launch may
  // not have been waited for yet — sequences only grow per workspace)
  r.posts = r.chunks = 0;
  // kernel arguments: ResDev*, ResHost*, table, table_bytes, then the code-object-v5 hidden block
  struct {
    ResDev* d;
    ResHost* h;
    const void* table;
    uint32_t table_bytes;
  } args{r.d, r.h_dev, table, table_bytes};
  const size_t hid = (sizeof(args) + 7) & ~(size_t)7;
  // (the kernel reads none of the code-object-v5 hidden arguments, so its kernarg segment may end
  // after the explicit ones: the hidden block is written anyway, into the 512-B region)
  if ((r.k->kernarg_size != hid + 256 && r.k->kernarg_size > hid) || hid + 256 > 512)
    throw Error(GCK_E_DEVICE, "engine invariant violated: resident join kernarg layout");
  auto* img = static_cast<unsigned char*>(r.kernarg);
  std::memset(img, 0, hid + 256);
  std::memcpy(img, &args, sizeof(args));
  const uint32_t bc[3] = {r.blocks, 1u, 1u};
  const uint16_t gs[3] = {(uint16_t)kBlock, 1u, 1u};
  const uint16_t dims = 1;
  std::memcpy(img + hid, bc, sizeof(bc));
  std::memcpy(img + hid + 12, gs, sizeof(gs));
  std::memcpy(img + hid + 64, &dims, 2);
  hsa_signal_store_relaxed(r.sig, 1);
  const uint64_t idx = hsa_queue_add_write_index_screlease(r.q, 1);
  while (idx - hsa_queue_load_read_index_scacquire(r.q) >= r.q->size) __builtin_ia32_pause();
  auto* p = static_cast<hsa_kernel_dispatch_packet_t*>(r.q->base_address) + (idx & (r.q->size - 1));
  p->workgroup_size_x = (uint16_t)kBlock;
  p->workgroup_size_y = 1;
  p->workgroup_size_z = 1;
  p->reserved0 = 0;
  p->grid_size_x = r.blocks * kBlock;
  p->grid_size_y = 1;
  p->grid_size_z = 1;
  p->private_segment_size = r.k->priv;
  p->group_segment_size = r.k->group;
  p->kernel_object = r.k->object;
  p->kernarg_address = r.kernarg;
  p->reserved2 = 0;
  p->completion_signal = r.sig;
  const uint16_t header = (uint16_t)((HSA_PACKET_TYPE_KERNEL_DISPATCH << HSA_PACKET_HEADER_TYPE) |
                                     (HSA_FENCE_SCOPE_SYSTEM << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) |
                                     (HSA_FENCE_SCOPE_SYSTEM << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE));
  const uint16_t setup = 1u << HSA_KERNEL_DISPATCH_PACKET_SETUP_DIMENSIONS;
  __atomic_store_n(reinterpret_cast<uint32_t*>(p), (uint32_t)header | ((uint32_t)setup << 16), __ATOMIC_RELEASE);
  hsa_signal_store_screlease(r.q->doorbell_signal, (hsa_signal_value_t)idx);
  r.running = true;
  r.table = table;
  r.table_bytes = table_bytes;
  r.launches++;
}

// Posts a closure-join request (the workspace's arguments `j`, `blocks` chunks of 128 checks).
static void res_post(Engine& e, Workspace& w, const CjArgs& j, uint32_t blocks) {
  ResState& r = *e.res;
  if (w.ws_index >= kResSlots) throw Error(GCK_E_DEVICE, "engine invariant violated: resident slot");
  std::lock_guard<std::mutex> lk(r.mu);
  if (r.running && (r.table != j.table || r.table_bytes != j.table_bytes || r.chunks + blocks > kResMaxChunks ||
                    r.posts + 1 >= 0x7FFFFFFFu || __atomic_load_n(&r.h->dead, __ATOMIC_ACQUIRE))) {
    if (r.inflight && (!res_device_idle(r) || __atomic_load_n(&r.h->dead, __ATOMIC_ACQUIRE)))
      throw Error(GCK_E_DEVICE, std::string("engine invariant violated: resident launch change with requests in flight (") +
                                    (r.table != j.table || r.table_bytes != j.table_bytes ? "table " : "") +
                                    (r.chunks + blocks > kResMaxChunks ? "chunks " : "") +
                                    (__atomic_load_n(&r.h->dead, __ATOMIC_ACQUIRE) ? "dead " : "") + "posts=" +
                                    std::to_string(r.posts) + " consumed=" + std::to_string(r.h->consumed) +
                                    " inflight=" + std::to_string(r.inflight) + " why=" + std::to_string(r.h->why[0]) +
                                    "," + std::to_string(r.h->why[1]) + "," + std::to_string(r.h->why[2]) + "," +
                                    std::to_string(r.h->why[3]) + ")");
    res_seal_locked(r);
  }
  if (!r.running) res_launch(e, r, j.table, j.table_bytes);
  const uint32_t slot = w.ws_index;
  ResArgs& ra = r.h->slots[slot];
  ra.a = j;
  ra.ctr = w.ctr;
  ra.done = &r.h_dev->done[slot][0];
  ra.seq = ++w.res_seq;
  r.seq_posted[slot] = ra.seq;
  ResPost& rp = r.h->ring[r.posts % kResRing];
  rp.slot = slot;
  rp.start = r.chunks;
  rp.n_chunks = blocks;
  rp.post = r.posts;
  r.chunks += blocks;
  r.posts++;
  __atomic_store_n(&r.h->posted, r.posts, __ATOMIC_RELEASE);
  r.inflight++;
  r.last = std::chrono::steady_clock::now();
  w.b_res = true;
}

// Waits for the workspace's posted request (its completion word reaching its sequence).
static void res_wait(Engine& e, Workspace& w) {
  ResState& r = *e.res;
  const uint32_t* done = &r.h->done[w.ws_index][0];
  const auto t0 = std::chrono::steady_clock::now();
  for (uint64_t it = 1; __atomic_load_n(done, __ATOMIC_ACQUIRE) != w.res_seq; ++it) {
    if ((it & 4095) == 0) {
      const bool dead = __atomic_load_n(&r.h->dead, __ATOMIC_ACQUIRE) != 0;
      if (dead || std::chrono::steady_clock::now() - t0 > std::chrono::seconds(30)) {
        std::lock_guard<std::mutex> lk(r.mu);
        r.inflight--;
        w.b_res = false;
        throw Error(GCK_E_DEVICE, dead ? "the resident join retired with a request posted" :
                                         "a resident join request did not finish in 30 s");
      }
    }
    __builtin_ia32_pause();
  }
  std::lock_guard<std::mutex> lk(r.mu);
  r.inflight--;
  r.last = std::chrono::steady_clock::now();
}

// Before anything a running launch reads changes (the snapshot, the workspaces) or goes: seal it.
static void res_drain(Engine& e) {
  if (!e.res) return;
  std::lock_guard<std::mutex> lk(e.res->mu);
  res_seal_locked(*e.res);
}

static void res_free(Engine& e) {
  if (!e.res) return;
  ResState* r = e.res;
  r->stop.store(true);
  if (r->keeper.joinable()) r->keeper.join();
  try {
    std::lock_guard<std::mutex> lk(r->mu);
    res_seal_locked(*r);
  } catch (const Error&) {
  }
  (void)hsa_signal_destroy(r->sig);
  (void)hsa_queue_destroy(r->q);
  (void)hipHostFree(r->h);
  (void)hipHostFree(r->kernarg);
  (void)hipFree(r->d);
  (void)hipStreamDestroy(r->st);
  delete r;
  e.res = nullptr;
}
