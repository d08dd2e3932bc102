// closure.inc — the closure-join stage of a check batch (included by engine.hip before bidir.inc).
//
// The commonest shape of a nested-group permission (SURVEY §8d config 4; Zanzibar's "Leopard"
// pattern) is
//     definition group { relation member: user | group#member }
//     definition doc   { relation viewer: group#member   permission view = viewer }
// A check doc:R#view@user:u is HAS iff some group g that lists u directly is one of R's viewer
// groups V(R), or has one of them among its ancestors (the ancestor closure bidir.inc builds for
// the self-recursive relation). With no caveat, expiration or wildcard on the way and every walk
// below the depth budget (the root is NF_BIDIR), that is the whole of SpiceDB's answer — HAS iff
// a path exists — so such a check skips the level-synchronous search:
//
//   round 1  the item; the row extents of R in the resource's group CSR and of u in the
//            transposed direct-member CSR (u -> the groups listing it), from an LDS table
//   round 2  V(R) (at most kCjV ids, into LDS) and G(u): one (check, g) task per lane slot,
//            kCjK per lane in flight
//   round 3  a 256-bit Bloom signature of {g} + anc(g) per task, tested against V(R)
//   round 4  signature hits only: g == v, or the closure-index probe "v is an ancestor of g"
//
// A check of another shape, or whose rows exceed the limits, goes on a deferred list that the
// wave-bundle kernel reads on the device (BundleArgs::idx / n_dev): no host round trip.
//
// Eligible roots (build_closure_join, from build_bidir): a forward node p that is NF_BIDIR and
// reaches through single computed usersets either (a) a relation n whose only item is the
// userset kind m of a self-recursive relation m with an ancestor closure — V(R) = row R of n's
// CSR — or (b) m itself — V(R) = {R}; m's items are its recursive userset kind and direct
// subject kinds (plain CSRs) only. Subjects: an object of a type m lists directly (G = its row
// of that kind's transposed CSR) or the userset x#m (G = {x}).

constexpr int kCjV = 8;            // ids of V(R) a check may have (more: deferred)
constexpr uint32_t kCjG = 512;     // groups of G(u) a check may have (more: deferred)
constexpr int kCjK = 2;            // tasks per lane in flight (the task rounds hold the kernel's register peak: 2 keeps it at 76 VGPRs)
constexpr int kCjL = 8;            // cover-list tasks per lane in flight (list round)
constexpr uint32_t kSigWords = 8;  // 256-bit signature per group
constexpr uint32_t kCjLdsBytes = 6144;       // the largest table staged in LDS
constexpr uint32_t kCjLdsBytesSmall = 2048;  // ... by the variant for small schemas (6 blocks per CU)
// slot fast path (below): entries a user / resource slot holds inline
// cover entries a user slot holds inline: 32-bit preorder numbers, or 24-bit ones when the
// hierarchy has at most 2^24 groups (the snapshot picks; slot_cap)
// (the user slot's layout — kUSlotWords, slot_cap, kSlotOverflow, kSlotList and a listed slot's
// inline entries and window — is slot_pack.hpp's)
constexpr int kSlotG = 15;             // at 32 bits (the decision loop's bound is slot_cap<BITS>)
constexpr int kSlotGMax = 20;
constexpr int kSlotV = 7;              // intervals of a resource's groups V(R) (more: the task rounds)
constexpr uint32_t kCoverMax = 15;     // cover entries per group (more: the group overflows)
constexpr uint32_t kDSlotWords = 16;   // 64 B per resource: count, (pre, end) per group
// half slots: what the first 32 B of a slot hold — the cover entries in words 1-7 (9 at 24 bits, 7
// at 32) and the intervals in words 2-7 (3). The rest of a user slot is all ones then (unused
// entries), the rest of a resource slot zero (empty intervals).
template <int BITS> constexpr uint32_t slot_half_cap() { return BITS == 24 ? 9u : 7u; }
constexpr uint32_t kSlotHalfV = 3;
static_assert(kFrontV == kSlotHalfV, "a front holds what half a resource slot holds");

struct CjEntry {  // one (eligible root, subject type): everything a check needs, flat (64 B)
  const uint32_t* v_off;   // R's groups (null: V(R) = {R})
  const uint32_t* v_nbr;
  const uint32_t* t_off;   // the subject type's transposed direct-member CSR (null: none; the
  const uint32_t* t_nbr;   // userset subject x#m is always taken)
  const uint32_t* sig;     // kSigWords per object of m's type
  const unsigned long long* anc_hash;  // membership index of the ancestor closure
  unsigned long long anc_bmask;        // its bucket mask
  uint32_t v_rows, t_rows;
  const uint32_t* uslot;   // slot fast path (null: none): kUSlotWords per subject (t_rows)
  const uint32_t* dslot;   // kDSlotWords per resource (v_rows)
  const uint32_t* ulist;   // the cover lists of users whose covers exceed a slot (null: none)
  const uint32_t* dfront;  // kFrontWords per resource: the slots' 16-B fronts (slot_pack.hpp; null: none — a
                           // 32-bit snapshot, GCK_DEBUG_CJ_FRONT=0)
};
static_assert(sizeof(CjEntry) == 96, "CjEntry layout");

struct CjMeta {  // per eligible root
  uint16_t mtype, mrel;   // the self-recursive relation m
  uint16_t rtype, pad;    // the root's resource type
  uint32_t m_rows;        // objects of m's type the hierarchy's labels cover (bidir.inc)
};

// The join's arguments. The kernel's kernarg segment is (Ctx, CjArgs); every wave of every batch
// reads its arguments through the scalar cache, which each dispatch's acquire has invalidated, so
// each 64-B line of the segment a wave touches before its slot loads is a serial miss. Everything
// the slot fast path reads therefore lies in ONE line — CjArgs bytes 40..103, kernarg 0x180..0x1bf
// (CjHot below, read once at entry as one 16-dword scalar load) — and the fields around it are read
// only inside the rare branches that use them (CjKernargs::cold). sizeof stays 184.
struct CjArgs {
  // ---- cold, bytes 0..39 ----
  uint32_t* deferred;      // indices of the checks left to the bundle stages
  unsigned* n_deferred;
  unsigned long long* timing;  // GCK_DEBUG_TIMING (TIMING=1 builds): kCjTimingWords per wave
  // the publication of a device batch (k_publish's work, done by the last block to finish; null
  // h_out: k_publish follows): pub_words counter words, read and zeroed, to h_out, then seq to
  // h_out[pub_words]; `done` (zero between batches) counts the finished blocks
  unsigned* pub;
  unsigned* h_out;
  // ---- the hot line, bytes 40..103 (CjHot has the same layout) ----
  const gck_item* items;
  uint8_t* out_perm;
  int32_t* out_err;
  const unsigned char* table;  // root[n_fwd] u16 (0xFFFF: not eligible), meta[n_desc], entries[n_desc][n_types]
  uint32_t n;
  uint32_t n_fwd, n_types;
  uint32_t table_bytes;        // a multiple of 16 (the table is staged in 16-B chunks; cj_table_bytes)
  uint32_t o_meta, o_entries;  // byte offsets in `table`
  // kPubCoherent (results written through the L2: engine-stream batches published by the join),
  // kPubBySignal, and what the kernel would otherwise learn from a cold pointer's null test
  // (kCjUniform ...: set by cj_seal once the pointers are final)
  uint32_t mode;
  // a list batch (below): kListOn | kListSubject | kListRange, 0 otherwise. The word lies in the hot
  // line's padding, but the kernel never reads it there: cj_seal turns it into mode bits
  uint32_t list;
  // ---- cold, bytes 104..183 ----
  unsigned* done;
  // host items read in place (a zero-copy batch): an item whose context_slot exceeds slot_limit
  // fails the request — the first such index lands in *bad_slot (DevCounters::bad_slot); null: no check
  unsigned* bad_slot;
  // a uniform batch (gck_check_bulk_uniform; null pairs: `items`): every check is the header words
  // u_rp (resource_type | permission << 16), u_ss (subject_type | subject_relation << 16), u_ctx
  // (context slot) and its (resource id, subject id) pair; its result is 2 bits of out_packed (32
  // checks per word). A check left to the bundle stages keeps bits 0, and its item goes to
  // items_out[i], where those stages read it (they answer into out_perm / out_err).
  const uint32_t* pairs;
  unsigned long long* out_packed;
  gck_item* items_out;
  uint32_t pub_words, seq;
  uint32_t slot_limit;
  uint32_t n_desc;
  // a shaped batch (gck_check_bulk_shaped; kCjShaped, with `pairs`): check k's header is
  // shapes[shape_of[k]] — a table of n_shapes <= GCK_MAX_SHAPES 16-B entries in device-visible
  // memory of the workspace, and one index byte per check beside the pairs. An index >= n_shapes is
  // clamped before the lookup and fails the request through *bad_slot (the check's context slot
  // reads as 0xFFFFFFFF there). The pointers lie over the header words a shaped batch does not use.
  union {
    struct {
      uint32_t u_rp, u_ss, u_ctx;
      uint32_t u_fixed;  // a list batch (below): the fixed id
    };
    struct {
      const uint8_t* shape_of;
      const gck_uniform* shapes;
    };
  };
  uint32_t n_shapes;  // 0: not shaped
  // a cross batch (gck_check_bulk_cross; kCjGrid, with `pairs`): `pairs` is the workspace's id block
  // — the tile's `cols` resource ids, then its subject ids from word cross_sub_off(cols) — and check
  // i of the n = rows * wpr * 32 (wpr = ceil(cols / 32)) is row (i / 32) / wpr, column
  // 32 * ((i / 32) % wpr) + i % 32 (cross_rc); a column >= cols is padding: the lane is idle and its
  // result bits are 0. The header is u_rp / u_ss / u_ctx. 0: not a cross batch.
  // A list batch (gck_check_bulk_list; kCjList, `list` != 0, never shaped nor a cross batch): check i
  // is the header, the fixed id u_fixed on one side — the subject's, or with kListSubject the
  // resource's — and on the other the 4-B id pairs[i], or with kListRange (null `pairs`) the id
  // cols + i: the word is then the range's first id, not a tile width.
  uint32_t cols;
};
// CjArgs::list / LjArgs::list
constexpr uint32_t kListOn = 1u;       // a list batch
constexpr uint32_t kListSubject = 2u;  // the subject id varies (the fixed id is the resource's)
constexpr uint32_t kListRange = 4u;    // the varying id of check i is cols + i (no id list)
// CjArgs::mode beside kPubCoherent | kPubBySignal (engine.hip)
constexpr uint32_t kCjUniform = 4u;   // pairs != null, or a list batch's range
constexpr uint32_t kCjBadSlot = 8u;   // bad_slot != null
constexpr uint32_t kCjSelfPub = 16u;  // h_out != null
constexpr uint32_t kCjTimed = 32u;    // timing != null
constexpr uint32_t kCjShaped = 64u;   // n_shapes != 0 (with kCjUniform)
constexpr uint32_t kCjGrid = 128u;    // cols != 0 (with kCjUniform, never with kCjShaped or kCjList)
constexpr uint32_t kCjListShift = 8u;  // `list` (with kCjUniform): kListOn, kListSubject, kListRange as bits 8..10
constexpr uint32_t kCjList = kListOn << kCjListShift;
constexpr uint32_t kCjListSub = kListSubject << kCjListShift;
constexpr uint32_t kCjRange = kListRange << kCjListShift;

struct CjHot {  // the hot line as the kernel holds it (scalar registers)
  const gck_item* items;
  uint8_t* out_perm;
  int32_t* out_err;
  const unsigned char* table;
  uint32_t n, n_fwd, n_types, table_bytes, o_meta, o_entries, mode, hot_pad;
};
constexpr size_t kCjHotOff = 40;
static_assert(sizeof(CjArgs) == 184, "CjArgs size (tests/test_aql_codeobject.py, aql.inc kBuildId)");
static_assert(sizeof(CjHot) == 64 && offsetof(CjArgs, items) == kCjHotOff && offsetof(CjArgs, done) == kCjHotOff + 64,
              "CjArgs hot line");
static_assert(offsetof(CjArgs, out_perm) - kCjHotOff == offsetof(CjHot, out_perm) &&
                  offsetof(CjArgs, out_err) - kCjHotOff == offsetof(CjHot, out_err) &&
                  offsetof(CjArgs, table) - kCjHotOff == offsetof(CjHot, table) &&
                  offsetof(CjArgs, n) - kCjHotOff == offsetof(CjHot, n) &&
                  offsetof(CjArgs, n_fwd) - kCjHotOff == offsetof(CjHot, n_fwd) &&
                  offsetof(CjArgs, n_types) - kCjHotOff == offsetof(CjHot, n_types) &&
                  offsetof(CjArgs, table_bytes) - kCjHotOff == offsetof(CjHot, table_bytes) &&
                  offsetof(CjArgs, o_meta) - kCjHotOff == offsetof(CjHot, o_meta) &&
                  offsetof(CjArgs, o_entries) - kCjHotOff == offsetof(CjHot, o_entries) &&
                  offsetof(CjArgs, mode) - kCjHotOff == offsetof(CjHot, mode),
              "CjHot mirrors CjArgs bytes 40..103");
static_assert((sizeof(Ctx) + kCjHotOff) % 64 == 0, "the hot line is one 64-B line of the (Ctx, CjArgs) kernarg segment");

// The mode bits that stand for a cold pointer's null test, once the pointers are final (before
// the launch, the dispatch or the post).
inline void cj_seal(CjArgs& j) {
  const uint32_t list = j.list & kListOn ? j.list & (kListOn | kListSubject | kListRange) : 0u;
  j.mode = (j.mode & (kPubCoherent | kPubBySignal)) | (j.pairs || list ? kCjUniform : 0u) | (j.bad_slot ? kCjBadSlot : 0u) |
           (j.h_out ? kCjSelfPub : 0u) | (j.timing ? kCjTimed : 0u) | (j.pairs && j.n_shapes && !list ? kCjShaped : 0u) |
           (j.pairs && !j.n_shapes && j.cols && !list ? kCjGrid : 0u) | list << kCjListShift;
}
// The staged bytes of a table of `bytes` bytes (its device buffer is allocated to this size).
constexpr uint32_t cj_table_bytes(size_t bytes) { return (uint32_t)((bytes + 15) & ~(size_t)15); }

// How cj_block reads a request's arguments: the hot line by value, the rest through cold() inside
// the branches that need it.
// k_closure_join: the kernarg segment itself. The segment pointer goes through an empty asm, so
// that the compiler cannot prove the loads behind it safe to hoist: a cold field's scalar load
// (and its wait) stays in its branch instead of joining the entry's.
#define GCK_CONST __attribute__((address_space(4)))
typedef uint32_t u32x16_a8 __attribute__((ext_vector_type(16), aligned(8)));
struct CjKernargs {
  CjHot h;
  static constexpr bool kLists = true;  // a dispatched join takes list batches (cj_block)
  __device__ __forceinline__ static const GCK_CONST unsigned char* seg() {
    const GCK_CONST unsigned char* p = (const GCK_CONST unsigned char*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
  }
  __device__ __forceinline__ void load_hot() {
    const u32x16_a8 v = *(const GCK_CONST u32x16_a8*)((const GCK_CONST unsigned char*)__builtin_amdgcn_kernarg_segment_ptr() +
                                                      sizeof(Ctx) + kCjHotOff);
    __builtin_memcpy(&h, &v, sizeof(h));
  }
  __device__ __forceinline__ const GCK_CONST CjArgs* cold() const { return (const GCK_CONST CjArgs*)(seg() + sizeof(Ctx)); }
  __device__ __forceinline__ DevCounters* ctr() const {
    return *(DevCounters* const GCK_CONST*)(seg() + offsetof(Ctx, ctr));
  }
  // the batch's block count: gridDim.x, the first word of the code object's hidden arguments
  // (hidden_block_count_x; tests/test_aql_codeobject.py) — read like a cold field, by the
  // last-block publication only
  __device__ __forceinline__ uint32_t nblk() const {
    const GCK_CONST uint32_t* p = (const GCK_CONST uint32_t*)__builtin_amdgcn_implicitarg_ptr();
    asm volatile("" : "+s"(p));
    return p[0];
  }
};
// A resident join's chunk (resident.inc): the request's arguments are in registers already.
struct CjLocalArgs {
  CjHot h;
  // (list batches are always dispatched — engine.hip closure_join_start — so the resident kernel
  // compiles their branches out and keeps its registers)
  static constexpr bool kLists = false;
  const CjArgs* a;
  DevCounters* c;
  uint32_t n_chunks;
  __device__ __forceinline__ uint32_t nblk() const { return n_chunks; }
  __device__ __forceinline__ const CjArgs* cold() const { return a; }
  __device__ __forceinline__ DevCounters* ctr() const { return c; }
};
__device__ __forceinline__ CjHot cj_hot(const CjArgs& a) {
  CjHot h;
  __builtin_memcpy(&h, reinterpret_cast<const unsigned char*>(&a) + kCjHotOff, sizeof(h));
  return h;
}

// A uniform batch's check i (CjArgs::pairs): the header and its id pair.
__device__ __forceinline__ gck_item uniform_item(uint32_t rp, uint32_t ss, uint32_t ctx, uint32_t res, uint32_t sub) {
  gck_item it;
  it.resource_type = (uint16_t)rp;
  it.permission = (uint16_t)(rp >> 16);
  it.resource_id = res;
  it.subject_type = (uint16_t)ss;
  it.subject_relation = (uint16_t)(ss >> 16);
  it.subject_id = sub;
  it.context_slot = ctx;
  return it;
}

// A cross batch's id block (CjArgs::cols): the word at which the subject ids begin — behind the
// tile's resource ids, on a 16-B line of its own (the host rewrites the block line by line).
__host__ __device__ constexpr uint32_t cross_sub_off(uint32_t cols) { return (cols + 3u) & ~3u; }
// ... and the (row, column) of the check whose result is bit pair `bit` of the tile's word `word`
// (wpr words per row). The join calls it with a wave-uniform word: a scalar division.
__host__ __device__ __forceinline__ void cross_rc(uint32_t word, uint32_t bit, uint32_t wpr, uint32_t& row, uint32_t& col) {
  row = word / wpr;
  col = (word - row * wpr) * 32u + bit;
}
// A cross batch's check, read again by (row, column) by the rare check the join leaves to the
// bundle stages: its resource id and its subject id from the id block.
__device__ __forceinline__ void cross_ids_again(const uint32_t* ids, uint32_t cols, uint32_t i, uint32_t& res, uint32_t& sub) {
  uint32_t row, col;
  cross_rc(i >> 5, i & 31u, (cols + 31u) >> 5, row, col);
  res = *(const GCK_GLOBAL uint32_t*)(ids + col);
  sub = *(const GCK_GLOBAL uint32_t*)(ids + cross_sub_off(cols) + row);
}

// A list batch's check i (CjArgs::list), built again by the rare check the join leaves to the
// bundle stages: its varying id read again — or, in range form, computed again — and the fixed id
// on the other side.
__device__ __forceinline__ void list_ids_again(const uint32_t* ids, uint32_t list, uint32_t first, uint32_t fixed, uint32_t i,
                                               uint32_t& res, uint32_t& sub) {
  const uint32_t v = (list & kListRange) ? first + i : *(const GCK_GLOBAL uint32_t*)(ids + i);
  res = (list & kListSubject) ? fixed : v;
  sub = (list & kListSubject) ? v : fixed;
}

// The packed results of a uniform batch: lane l of a wave whose first check is w0 (a multiple of
// 32) holds the 2-bit result v of check w0 + l; lanes 0 and 32 store one word of 32 results each
// (one 8-B write per 32 checks: the words go across PCIe into the caller's pinned buffer). Every
// lane of the wave calls it.
__device__ __forceinline__ void packed_store(unsigned long long* out, uint32_t w0, uint32_t v, int lane, uint32_t cpw,
                                             uint32_t n) {
  uint32_t lo = (uint32_t)lane & 31u;
  uint32_t x0 = lo < 16u ? v << (2u * lo) : 0u, x1 = lo < 16u ? 0u : v << (2u * (lo - 16u));
#pragma unroll
  for (int o = 1; o < 32; o <<= 1) {
    x0 |= (uint32_t)__shfl_xor((int)x0, o, 64);
    x1 |= (uint32_t)__shfl_xor((int)x1, o, 64);
  }
  if (lo == 0u && (uint32_t)lane < cpw && w0 + (uint32_t)lane < n)
    out[(w0 + (uint32_t)lane) >> 5] = (unsigned long long)x0 | ((unsigned long long)x1 << 32);
}

// The request check of host items a zero-copy batch reads in place (include/gck.h: a context_slot
// beyond the call's contexts is GCK_E_INVALID_ARGUMENT): the wave's first offending item, kept as
// 0xFFFFFFFF - index by an atomic max so that the smallest index wins. Completed before the lane
// goes on (the block's publication reads the counters after the block barrier).
__device__ __forceinline__ bool check_slots(unsigned* bad, uint32_t limit, bool active, const gck_item& it,
                                            uint32_t w0, int lane) {
  const unsigned long long m = __ballot(active && it.context_slot > limit);
  if (m && lane == 0) {
    atomicMax(bad, 0xFFFFFFFFu - (w0 + (uint32_t)__ffsll((long long)m) - 1u));
    __builtin_amdgcn_s_waitcnt(0);
  }
  return m != 0;
}

// A join dispatched into an engine HSA queue (kPubBySignal): the packet's completion signal tells
// the host the batch has ended, so no block needs to learn that it is the last — the round trips
// of that protocol (an atomic arrival, then the counters read and zeroed with atomics) were ~4 us
// at the tail of every batch (DESIGN §3.4). Instead each block that deferred checks or touched a
// counter writes {deferred checks, counters touched} to its own slot in host memory (posted
// writes; the host sums the slots after the signal and reads the device counters only when a
// block touched them), and the deferred-list counter alternates between two words per batch,
// block 0 clearing the one the next batch will use (`clear`).
// (blk: the block's index in the batch — blockIdx.x, or a resident join's chunk)
__device__ __forceinline__ void block_summary(unsigned* slots, unsigned* clear, uint32_t deferred, uint32_t touched,
                                              uint32_t blk) {
  if (deferred | touched) {
    slots[2 * blk] = deferred;
    slots[2 * blk + 1] = touched;
  }
  if (blk == 0) __hip_atomic_store(clear, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ... with the two pointers read from the join's cold arguments only by the blocks that write
template <class A>
__device__ __forceinline__ void block_summary_cold(const A& a, uint32_t deferred, uint32_t touched, uint32_t blk) {
  if (deferred | touched) {
    unsigned* slots = a.cold()->h_out;
    slots[2 * blk] = deferred;
    slots[2 * blk + 1] = touched;
  }
  if (blk == 0) __hip_atomic_store(a.cold()->done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// per wave: {start, table staged, round 1 done, tasks done, end, tasks, probes, checks taken,
// items staged, slots and lists decided, slots decided, checks whose front said "read the slot"}
constexpr int kCjTimingWords = 12;

__device__ __forceinline__ void sig_bits(uint32_t v, uint32_t& b0, uint32_t& b1, uint32_t& b2) {
  const uint64_t h = mix64(0x9E3779B97F4A7C15ull ^ v);
  b0 = (uint32_t)h & 255u;
  b1 = (uint32_t)(h >> 8) & 255u;
  b2 = (uint32_t)(h >> 16) & 255u;
}

__device__ __forceinline__ void sig_set(uint32_t* s, uint32_t v) {
  uint32_t b0, b1, b2;
  sig_bits(v, b0, b1, b2);
  atomicOr(&s[b0 >> 5], 1u << (b0 & 31));
  atomicOr(&s[b1 >> 5], 1u << (b1 & 31));
  atomicOr(&s[b2 >> 5], 1u << (b2 & 31));
}

// Signature of every group g: the bits of g and of each ancestor in row g of the closure (one
// lane per closure entry, then one per row for g itself).
__global__ void __launch_bounds__(kBlock) k_sig_build(const uint32_t* __restrict__ off, const uint32_t* __restrict__ nbr,
                                                      uint32_t n_rows, unsigned long long n_edges,
                                                      uint32_t* __restrict__ sig) {
  __shared__ uint32_t rows[2];
  const unsigned long long e0 = (unsigned long long)blockIdx.x * kBlock;
  const unsigned long long e = e0 + threadIdx.x;
  if (e0 < n_edges) {  // block-uniform
    const uint32_t o = block_edge_row(off, n_rows, n_edges, e0, e < n_edges ? e : n_edges - 1, rows);
    if (e < n_edges) sig_set(sig + (size_t)o * kSigWords, nbr[e]);
  }
  const unsigned long long s = e - n_edges;
  if (e >= n_edges && s < n_rows) sig_set(sig + s * kSigWords, (uint32_t)s);
}

__device__ __forceinline__ bool sig_has(const uint32_t (&s)[kSigWords], uint32_t v) {
  uint32_t b0, b1, b2;
  sig_bits(v, b0, b1, b2);
  uint32_t w0 = 0, w1 = 0, w2 = 0;
#pragma unroll
  for (uint32_t k = 0; k < kSigWords; ++k) {  // selects: the array stays in registers
    w0 = (b0 >> 5) == k ? s[k] : w0;
    w1 = (b1 >> 5) == k ? s[k] : w1;
    w2 = (b2 >> 5) == k ? s[k] : w2;
  }
  return ((w0 >> (b0 & 31)) & (w1 >> (b1 & 31)) & (w2 >> (b2 & 31)) & 1u) != 0;
}

// ---- slot fast path ---------------------------------------------------------------------------
// The task rounds above cost a check a random read per group of the user (its signature) after
// two dependent reads of row extents and rows. The HBM is large enough to lay every check's
// inputs out where one read finds them (MI355X: 288 GB per GPU), and the group hierarchy has an
// exact, compact description of ancestry:
//
//   tree labels  a spanning forest of the hierarchy over each group's first parent and its
//                preorder interval [pre, end) per group: x is a tree ancestor of y, or y itself,
//                iff pre(x) <= pre(y) < end(x);
//   tree cover   per group g a few groups C(g) whose tree ancestors (themselves included) are
//                exactly g's ancestors and g: C(g) = {g} + the covers of g's parents, pruned of
//                every entry that is a tree ancestor of another (build_ancestors). A group with a
//                single parent whose cover is a single entry has C(g) = {g}; each non-tree parent
//                on the way up adds one entry. Proof of exactness: an upward path from g ends, after
//                its last non-tree edge y -> p, in p's tree ancestors, and p is covered;
//   user slot    64 B per user: the preorder numbers of the covers of all its groups — or, when
//                they exceed the slot even sorted and without duplicates, 18 of them (13 at 32
//                bits), the open range in which the others lie, and where the whole sorted list
//                lies in a list array (slot_pack.hpp: one more round for that user's check only
//                when neither the inline entries nor the range decide it);
//   resource slot 64 B per resource: the interval [pre(v), end(v)) of each of its groups v.
//
// A check reads its two slots together and is HAS iff some cover entry lies in some interval —
// exact, no signature, no probe. Users whose covers do not fit a slot, resources with more
// groups than a slot holds, and userset subjects take the task rounds unchanged.

// Covers of user u's groups: their total count, or kSlotOverflow when a group's cover overflowed
// or a group id is out of range.
__device__ __forceinline__ uint32_t user_cover_count(const uint32_t* t_off, const uint32_t* t_nbr, uint32_t u,
                                                     const uint32_t* lab, const uint32_t* cov_off, uint32_t n_groups) {
  const uint32_t b = t_off[u], n = t_off[u + 1] - b;
  uint32_t m = 0;
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t g = t_nbr[b + k];
    if (g >= n_groups || (lab[2 * (size_t)g] & kSlotOverflow)) return kSlotOverflow;
    m += cov_off[g + 1] - cov_off[g];
    if (m > kSlotCount) return kSlotOverflow;
  }
  return m;
}

// Entry k of a user slot (word 0 is the count): BITS-wide fields packed from bit 32.
template <int BITS, int K>
__device__ __forceinline__ uint32_t slot_entry(const uint32_t (&w)[kUSlotWords]) {
  if constexpr (BITS == 32) {
    return w[1 + K];
  } else {
    constexpr int off = 32 + K * BITS, wi = off / 32, sh = off % 32;
    uint32_t v = w[wi] >> sh;
    if constexpr (sh + BITS > 32) v |= w[wi + 1] << (32 - sh);
    return v & ((1u << BITS) - 1u);
  }
}

template <int BITS, int K>
__device__ __forceinline__ void slot_put(uint32_t (&w)[kUSlotWords], uint32_t x) {
  if constexpr (BITS == 32) {
    w[1 + K] = x;
  } else {
    constexpr int off = 32 + K * BITS, wi = off / 32, sh = off % 32;
    w[wi] |= x << sh;
    if constexpr (sh + BITS > 32) w[wi + 1] |= x >> (32 - sh);
  }
}

template <int BITS, int K = 0>
__device__ __forceinline__ void slot_put_at(uint32_t (&w)[kUSlotWords], uint32_t m, uint32_t x) {
  if constexpr (K < slot_cap<BITS>()) {
    if (m == (uint32_t)K) slot_put<BITS, K>(w, x);  // registers, no scratch
    slot_put_at<BITS, K + 1>(w, m, x);
  }
}

// The slot of a user whose `total` raw cover entries, more than a slot holds, were written to
// e = list + list_at (slot_pack.hpp): up to kSlotSortMax of them are sorted there and lose their
// duplicates — the user then gets an inline slot if they fit now (its list stays unused), and a
// listed slot with inline entries and a window over the sorted list otherwise. More: a plain list.
template <int BITS>
__device__ __forceinline__ void user_slot_listed(uint32_t* e, uint32_t total, uint32_t list_at, uint32_t* w) {
  if (total > kSlotSortMax) {
    slot_pack_plain_list(BITS, total, list_at, w);
    return;
  }
  slot_pack_sorted(BITS, e, slot_sort_unique(e, total), list_at, w);
}

// The slot of user u: the covers of its groups, inline, or in the list at `list_at` (kNone: no
// list, such a user overflows).
template <int BITS>
__device__ __forceinline__ void user_slot(const uint32_t* __restrict__ t_off, const uint32_t* __restrict__ t_nbr, uint32_t u,
                                          const uint32_t* __restrict__ lab, const uint32_t* __restrict__ cov_off,
                                          const uint32_t* __restrict__ cov_pre, uint32_t n_groups, uint32_t list_at,
                                          uint32_t* __restrict__ list, uint32_t* __restrict__ out_slot) {
  const uint32_t b = t_off[u], n = t_off[u + 1] - b;
  const uint32_t total = user_cover_count(t_off, t_nbr, u, lab, cov_off, n_groups);
  uint32_t w[kUSlotWords];
#pragma unroll
  for (uint32_t k = 0; k < kUSlotWords; ++k) w[k] = 0u;
  if (total & kSlotOverflow) {
    w[0] = kSlotOverflow;
  } else if (total > (uint32_t)slot_cap<BITS>()) {
    if (list_at != kNone && list) {
      uint32_t m = 0;
      for (uint32_t k = 0; k < n; ++k) {
        const uint32_t g = t_nbr[b + k];
        for (uint32_t c = cov_off[g]; c < cov_off[g + 1]; ++c) list[list_at + m++] = cov_pre[c];
      }
      uint32_t lw[kUSlotWords];  // (indexed by entry: memory, apart from the inline slot's registers)
      user_slot_listed<BITS>(list + list_at, total, list_at, lw);
#pragma unroll
      for (uint32_t k = 0; k < kUSlotWords; ++k) w[k] = lw[k];
    } else {
      w[0] = kSlotOverflow;
    }
  } else {
    uint32_t m = 0;
    for (uint32_t k = 0; k < n; ++k) {
      const uint32_t g = t_nbr[b + k];
      for (uint32_t c = cov_off[g]; c < cov_off[g + 1]; ++c) slot_put_at<BITS>(w, m++, cov_pre[c]);
    }
    w[0] = m;
    // unused entries are all ones: above every interval (the snapshot takes 24-bit entries only
    // while every preorder number and interval end is below 2^24 - 1), so the test needs no count
    for (uint32_t k = m; k < (uint32_t)slot_cap<BITS>(); ++k) slot_put_at<BITS>(w, k, kSlotUnused<BITS>);
  }
  uint4* out = reinterpret_cast<uint4*>(out_slot);
#pragma unroll
  for (uint32_t j = 0; j < kUSlotWords / 4; ++j) out[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
}

// One pass over every user (the random reads of its groups' labels and covers once): inline slots
// written; a user with more raw cover entries than a slot holds gets their number in len[u] (0 for
// everyone else) and a placeholder slot — k_user_lists then writes the lists at the scanned offsets
// and those users' slots whole (user_slot_listed, slot_pack.hpp: inline after all, or listed).
template <int BITS>
__global__ void __launch_bounds__(kBlock) k_user_slots_1p(const uint32_t* __restrict__ t_off, const uint32_t* __restrict__ t_nbr,
                                                          uint32_t n_users, const uint32_t* __restrict__ lab,
                                                          const uint32_t* __restrict__ cov_off,
                                                          const uint32_t* __restrict__ cov_pre, uint32_t n_groups,
                                                          uint32_t* __restrict__ slots, uint32_t* __restrict__ len) {
  const uint32_t u = blockIdx.x * kBlock + threadIdx.x;
  if (u >= n_users) return;
  const uint32_t total = user_cover_count(t_off, t_nbr, u, lab, cov_off, n_groups);
  const bool listed = !(total & kSlotOverflow) && total > (uint32_t)slot_cap<BITS>();
  len[u] = listed ? total : 0u;
  if (!listed) {
    user_slot<BITS>(t_off, t_nbr, u, lab, cov_off, cov_pre, n_groups, kNone, nullptr, slots + (size_t)u * kUSlotWords);
    return;
  }
  uint4* out = reinterpret_cast<uint4*>(slots + (size_t)u * kUSlotWords);
  out[0] = make_uint4(kSlotList | total, 0u, 0u, 0u);
  for (uint32_t j = 1; j < kUSlotWords / 4; ++j) out[j] = make_uint4(0u, 0u, 0u, 0u);
}

// The cover lists of the users k_user_slots_1p marked (len[u] > 0) at list_off[u], and their slots
// (user_slot_listed); without a list array (too large) those users overflow instead.
template <int BITS>
__global__ void __launch_bounds__(kBlock) k_user_lists(const uint32_t* __restrict__ t_off, const uint32_t* __restrict__ t_nbr,
                                                       uint32_t n_users, const uint32_t* __restrict__ cov_off,
                                                       const uint32_t* __restrict__ cov_pre, const uint32_t* __restrict__ len,
                                                       const uint32_t* __restrict__ list_off, uint32_t* __restrict__ list,
                                                       uint32_t* __restrict__ slots) {
  const uint32_t u = blockIdx.x * kBlock + threadIdx.x;
  if (u >= n_users || len[u] == 0u) return;
  uint32_t* w = slots + (size_t)u * kUSlotWords;
  if (!list) {
    w[0] = kSlotOverflow;
    return;
  }
  const uint32_t b = t_off[u], n = t_off[u + 1] - b, at = list_off[u];
  uint32_t m = 0;
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t g = t_nbr[b + k];
    for (uint32_t c = cov_off[g]; c < cov_off[g + 1]; ++c) list[at + m++] = cov_pre[c];
  }
  uint32_t lw[kUSlotWords];
  user_slot_listed<BITS>(list + at, m, at, lw);
  uint4* out = reinterpret_cast<uint4*>(w);
  for (uint32_t j = 0; j < kUSlotWords / 4; ++j) out[j] = make_uint4(lw[4 * j], lw[4 * j + 1], lw[4 * j + 2], lw[4 * j + 3]);
}

// The slots of the users ids[0, n) only (a Watch batch's, delta.inc), into staged[i]; their lists
// at list_off[i] (already offset past the lists the slot array's other users keep).
template <int BITS>
__global__ void __launch_bounds__(kBlock) k_user_slots_ids(const uint32_t* __restrict__ t_off, const uint32_t* __restrict__ t_nbr,
                                                           const uint32_t* __restrict__ ids, uint32_t n,
                                                           const uint32_t* __restrict__ lab, const uint32_t* __restrict__ cov_off,
                                                           const uint32_t* __restrict__ cov_pre, uint32_t n_groups,
                                                           const uint32_t* __restrict__ list_off, uint32_t* __restrict__ list,
                                                           uint32_t* __restrict__ staged) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  user_slot<BITS>(t_off, t_nbr, ids[i], lab, cov_off, cov_pre, n_groups, list_off ? list_off[i] : kNone, list,
                  staged + (size_t)i * kUSlotWords);
}

__global__ void __launch_bounds__(kBlock) k_user_list_len_ids(const uint32_t* __restrict__ t_off, const uint32_t* __restrict__ t_nbr,
                                                              const uint32_t* __restrict__ ids, uint32_t n,
                                                              const uint32_t* __restrict__ lab,
                                                              const uint32_t* __restrict__ cov_off, uint32_t n_groups,
                                                              uint32_t cap, uint32_t* __restrict__ len) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t m = user_cover_count(t_off, t_nbr, ids[i], lab, cov_off, n_groups);
  len[i] = (m & kSlotOverflow) || m <= cap ? 0u : m;
}

__global__ void __launch_bounds__(kBlock) k_add_u32(uint32_t* __restrict__ v, uint32_t n, uint32_t x) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) v[i] += x;
}

// Staged slots into their users' places (engine.hip device_publish).
__global__ void __launch_bounds__(kBlock) k_slot_scatter(uint32_t* __restrict__ slots, const uint32_t* __restrict__ staged,
                                                         const uint32_t* __restrict__ ids, uint32_t n) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint4* src = reinterpret_cast<const uint4*>(staged + (size_t)i * kUSlotWords);
  uint4* dst = reinterpret_cast<uint4*>(slots + (size_t)ids[i] * kUSlotWords);
#pragma unroll
  for (uint32_t j = 0; j < kUSlotWords / 4; ++j) dst[j] = src[j];
}

// One thread per resource: the interval of each of its groups, and the slot's front (slot_pack.hpp).
__global__ void __launch_bounds__(kBlock) k_res_slots(const uint32_t* __restrict__ v_off, const uint32_t* __restrict__ v_nbr,
                                                      uint32_t n_res, const uint32_t* __restrict__ lab, uint32_t n_groups,
                                                      uint32_t* __restrict__ slots, uint32_t* __restrict__ fronts) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= n_res) return;
  const uint32_t b = v_off[r], n = v_off[r + 1] - b;
  uint32_t w[kDSlotWords];
#pragma unroll
  for (uint32_t k = 0; k < kDSlotWords; ++k) w[k] = 0u;
  bool ok = n <= (uint32_t)kSlotV;
#pragma unroll
  for (int k = 0; k < kSlotV; ++k) {
    if ((uint32_t)k >= n || !ok) continue;
    const uint32_t v = v_nbr[b + k];
    if (v >= n_groups) {
      ok = false;
      continue;
    }
    w[2 + 2 * k] = lab[2 * (size_t)v] & ~kSlotOverflow;
    w[3 + 2 * k] = lab[2 * (size_t)v + 1];
  }
  w[0] = ok ? n : kSlotOverflow;
  uint4* out = reinterpret_cast<uint4*>(slots + (size_t)r * kDSlotWords);
#pragma unroll
  for (uint32_t j = 0; j < kDSlotWords / 4; ++j) out[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
  uint32_t f[kFrontWords];
  front_pack(w, f);
  *reinterpret_cast<uint4*>(fronts + (size_t)r * kFrontWords) = make_uint4(f[0], f[1], f[2], f[3]);
}

template <int BITS, int K = 0>
__device__ __forceinline__ void slot_unpack(const uint32_t (&w)[kUSlotWords], uint32_t (&p)[kSlotGMax]) {
  if constexpr (K < slot_cap<BITS>()) {
    p[K] = slot_entry<BITS, K>(w);
    slot_unpack<BITS, K + 1>(w, p);
  }
}

// The entries the decision loop runs over for a slot with header w0.
template <int BITS>
__device__ __forceinline__ uint32_t slot_inline_count(uint32_t w0) {
  return (w0 & kSlotOverflow) ? 0u : (w0 & kSlotList) ? (uint32_t)slot_inline_cap<BITS>() : w0;
}

// The slot test of one check over its user slot w and resource slot d: 2 = HAS, 1 = NO,
// 3 = the user's covers are a list and neither its inline entries nor its window decide (the list
// round does), 0 = a slot overflowed (the task rounds decide). A listed slot (slot_pack.hpp) goes
// through the same loop as an inline one: its last two entry positions, the list's offset, count
// as unused, and beside each interval's entry tests stands the window's — can [lo, end) hold a
// point of the open range (lo1 - 1, hi) in which every omitted entry lies. The loops run to the
// wave's largest entry and interval counts (ng_max, nv_max: wave-uniform, so the bounds are scalar
// branches), every lane over all of them — unused entries are all ones and unused intervals empty,
// so neither can hit. One unsigned compare per (entry, interval): lo <= p < hi iff p - lo < hi - lo.
template <int BITS>
__device__ __forceinline__ uint32_t slot_decide_wave(const uint32_t (&w)[kUSlotWords], const uint32_t (&d)[kDSlotWords],
                                                     uint32_t ng_max, uint32_t nv_max) {
  if ((d[0] | w[0]) & kSlotOverflow) return 0u;
  const bool listed = (w[0] & kSlotList) != 0u;
  uint32_t p[kSlotGMax];
  slot_unpack<BITS>(w, p);
  constexpr int kIn = slot_inline_cap<BITS>();
  if (listed) p[kIn] = p[kIn + 1] = kSlotUnused<BITS>;
  const uint32_t hi = (w[0] & kSlotHiOpen) ? 0xFFFFFFFFu : p[0];
  const uint32_t lo1 = (w[0] & kSlotLoOpen) ? 0u : p[kIn - 1] + 1u;
  bool hit = false, open = false;  // (open: an interval reaches into the window; empty intervals are [0, 0): never)
#pragma unroll
  for (int j = 0; j < kSlotV; ++j) {
    if ((uint32_t)j >= nv_max) break;
    const uint32_t lo = d[2 + 2 * j], len = d[3 + 2 * j] - lo;
    open |= lo < hi && d[3 + 2 * j] > lo1;
#pragma unroll
    for (int k = 0; k < slot_cap<BITS>(); ++k) {
      if ((uint32_t)k >= ng_max) break;
      hit |= p[k] - lo < len;
    }
  }
  return hit ? 2u : (listed && open) ? 3u : 1u;
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// A shaped batch's check (CjArgs::shapes): its table entry e (16 B: gck_uniform) and its id pair. `bad`:
// its index byte was beyond the table (the entry is the clamped one) — the item then carries a
// context slot no call has, which check_slots reports as the request's error.
__device__ __forceinline__ gck_item shaped_item(const u32x4 e, bool bad, uint32_t res, uint32_t sub) {
  return uniform_item(e.x, e.y, bad ? 0xFFFFFFFFu : e.z, res, sub);
}
// ... read again from global memory, by the rare check the join leaves to the bundle stages (the
// index clamped as in the join; the request has failed already when it was out of range)
__device__ __forceinline__ gck_item shaped_item_again(const uint8_t* shape_of, const gck_uniform* shapes, uint32_t n_shapes,
                                                      uint32_t i, uint32_t res, uint32_t sub) {
  const uint32_t sb = *(const GCK_GLOBAL uint8_t*)(shape_of + i);
  const u32x4 e = *(const GCK_GLOBAL u32x4*)(shapes + min(sb, n_shapes - 1u));
  return shaped_item(e, false, res, sub);
}

// slot lines are read once per check and never again by the batch: nontemporal loads
// (tools/slot_probe: 8 % more random lines/s at three batches' worth of waves)
__device__ __forceinline__ u32x4 slot_load(const GCK_GLOBAL u32x4* p) {
#if GCK_SLOT_TEMPORAL
  return *p;
#else
  return __builtin_nontemporal_load(p);
#endif
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {  // wave-uniform (scalar register)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
constexpr uint32_t kSlotLines = 2;                           // per check: the user line, the resource line
constexpr uint32_t kCheckWords = kUSlotWords + kDSlotWords;  // staged per check (32 words)
constexpr uint32_t kStagePhases = 2;                         // the slots are staged half a wave at a time
constexpr uint32_t kStageWords = kCheckWords / kStagePhases; // LDS stage words per check of the wave

// One wavefront per 64 checks, 4 per block. TAB: the LDS bytes of the staged table (the launch
// picks the smallest variant that holds it: LDS per block decides how many blocks share a CU).
// CPW: checks per wave (64, or 32: twice the waves, each waiting for the slowest of 64 lines
// instead of 128).
// The join of one block of checks: blk is the block's index in the batch (blockIdx.x, or a resident
// join's chunk, resident.inc) and ax.nblk() the batch's block count; load_tab: stage the table in LDS (a
// resident join stages it once per launch: the same static LDS every call). Counters: ax.ctr().
// Returns (every thread) the checks the block left to the bundle stages.
// Arguments: ax (CjKernargs or CjLocalArgs above) — `a` is its hot line, everything else is read
// through ax.cold() / ax.ctr() where it is used; t_start: the wave's first timestamp (timing builds).
template <int BITS, uint32_t TAB, uint32_t CPW, bool HALF, class A>
__device__ __forceinline__ uint32_t cj_block(const A& ax, const uint32_t blk, const bool load_tab,
                                         const unsigned long long t_start) {
  static_assert(CPW == 64 || CPW == 32, "checks per wave");
  static_assert(!HALF || CPW == 32, "half slots: 32 checks per wave");
  const CjHot& a = ax.h;
  const bool timed = GCK_BUNDLE_TIMING && (a.mode & kCjTimed);
  __shared__ __attribute__((aligned(16))) unsigned char s_tab[TAB];
  __shared__ uint32_t s_nv[kWaves][64], s_excl[kWaves][65], s_hit[kWaves][64];
  __shared__ unsigned long long s_gp[kWaves][64];  // task base: &t_nbr[row start], or the group itself
  __shared__ uint16_t s_e[kWaves][64];             // the check's CjEntry
  // the wave's items (64 x 20 B) and its checks' slots, fetched line by line by the whole wave:
  // one 16-B chunk per lane, four lanes per 64-B line, so that every line is one memory request.
  // One 4-KB LDS region per wave, used in turn (each use ends before the next begins, in wave
  // order): the items (64 x 5 words); the slot addresses (64 x 2 x u64); the slots, half a wave
  // of checks at a time (kStagePhases x 32 checks x kCheckWords); the resource slots of the list
  // round (64 x kDSlotWords); the task rounds' V(R) (64 x kCjV). 4 KB instead of the 8 KB a
  // whole wave's slots take: 5 blocks per CU instead of 3, so more batches' waves share a CU.
  __shared__ __attribute__((aligned(16))) uint32_t s_stage[kWaves][64 * kStageWords];
  static_assert(64 * 5 <= 64 * kStageWords && 64 * kCjV <= 64 * kStageWords && 64 * 4 <= 64 * kStageWords &&
                    64 * kDSlotWords <= 64 * kStageWords && 64 * kCheckWords == kStagePhases * 64 * kStageWords,
                "LDS stage too small");
  uint32_t* const s_item_w = s_stage[threadIdx.x >> 6];                // items
  uint32_t* const s_slot_w = s_stage[threadIdx.x >> 6];                // slots
  uint32_t (*const s_v_w)[kCjV] = reinterpret_cast<uint32_t (*)[kCjV]>(s_stage[threadIdx.x >> 6]);  // V(R)
  unsigned long long* const s_ua = reinterpret_cast<unsigned long long*>(s_stage[threadIdx.x >> 6]);  // addresses
  unsigned long long* const s_da = s_ua + 64;
  const int wib = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // the wave's items of a full 32-check wave are requested before the table: both loads in flight
  // together, one memory round instead of two before the slots can be addressed
  const uint32_t w0 = (blk * kWaves + wib) * CPW;
  const bool uni = (a.mode & kCjUniform) != 0u;  // (a kernel argument: a scalar branch)
  const uint32_t item_bytes = w0 < a.n ? min(CPW, a.n - w0) * 20u : 0u;
  const bool items_early = !uni && CPW == 32 && ((uintptr_t)a.items & 15u) == 0 && item_bytes == CPW * 20u;
  u32x4 item_chunk{0u, 0u, 0u, 0u};
  if (items_early && lane < 40)
    item_chunk = *(const GCK_GLOBAL u32x4*)(reinterpret_cast<const unsigned char*>(a.items) + (size_t)w0 * 20u + lane * 16u);
  // a uniform batch: each lane its own check's 8-B pair, requested before the table as the items
  // are (into the same registers; not a cross batch's lanes: `pairs` is then the id block; nor a
  // list batch's: the id list, or null)
  const bool grid = (a.mode & kCjGrid) != 0u;
  const bool list = A::kLists && (a.mode & kCjList) != 0u;
  if (uni) {
    const uint32_t* pairs = ax.cold()->pairs;
    if ((uint32_t)lane < CPW && w0 + (uint32_t)lane < a.n && !(grid || list)) {
      const unsigned long long pr = *(const GCK_GLOBAL unsigned long long*)(pairs + 2ull * (w0 + (uint32_t)lane));
      item_chunk.x = (uint32_t)pr;
      item_chunk.y = (uint32_t)(pr >> 32);
    }
  }
  // a cross batch: in the same round the lane's resource id (32 consecutive words per result word:
  // one request) and its row's subject id (one address per result word) from the id block, into
  // the chunk's two spare registers (.z, .w; a shaped batch's index byte uses .z, and a cross batch
  // is never shaped) until the table's barrier — a branch of its own, shaped like the shaped
  // batch's below: as the other arm of the pair's load it made the compiler wait for the uniform
  // mode's pair before it issued the table's loads. A lane whose column is padding loads nothing
  // and stays idle (grid_on)
  bool grid_on = true;
  if (__builtin_expect(grid, 0)) {
    const auto cold = ax.cold();
    const uint32_t* ids = cold->pairs;
    const uint32_t cols = cold->cols, wpr = (cols + 31u) >> 5;
    uint32_t row, col;  // (the wave's first word: scalar; a wave of 64 checks holds two words)
    cross_rc((uint32_t)__builtin_amdgcn_readfirstlane((int)(w0 >> 5)), (uint32_t)lane & 31u, wpr, row, col);
    if (CPW == 64 && lane >= 32) {
      col += 32u;
      if (col >= wpr * 32u) col -= wpr * 32u, ++row;
    }
    grid_on = col < cols;
    if ((uint32_t)lane < CPW && w0 + (uint32_t)lane < a.n && grid_on) {
      item_chunk.z = *(const GCK_GLOBAL uint32_t*)(ids + col);
      item_chunk.w = *(const GCK_GLOBAL uint32_t*)(ids + cross_sub_off(cols) + row);
    }
  }
  // a list batch: in the same round the lane's one 4-B id (32 consecutive words per result word:
  // one request) — in range form computed, nothing loaded — into the chunk's spare register .z, the
  // fixed id into .w, until the table's barrier. A branch of its own for the cross batch's reason;
  // its arguments are read through cold() here, not with the hot line
  if (__builtin_expect(list, 0)) {
    const auto cold = ax.cold();
    const uint32_t* ids = cold->pairs;
    const uint32_t fixed = cold->u_fixed, first = cold->cols;
    if ((uint32_t)lane < CPW && w0 + (uint32_t)lane < a.n) {
      item_chunk.w = fixed;
      if (a.mode & kCjRange) item_chunk.z = first + w0 + (uint32_t)lane;
      else item_chunk.z = *(const GCK_GLOBAL uint32_t*)(ids + w0 + (uint32_t)lane);
    }
  }
  // a shaped batch: in the same round each check lane its index byte (32 consecutive bytes per
  // wave: one request) and lane l < n_shapes entry l of the shape table (<= 1 KB, the same for
  // every wave: L2-hot after the first). The entries go to the wave's own stage region, idle in
  // this mode until the slot addresses: each lane then reads its entry by index from LDS — no
  // dependent global round, no block barrier beyond the table's.
  const bool shaped = (a.mode & kCjShaped) != 0u;
  uint32_t n_shapes = 0;
  u32x4 shape_ent{0u, 0u, 0u, 0u};
  if (__builtin_expect(shaped, 0)) {
    const auto cold = ax.cold();
    const uint8_t* shape_of = cold->shape_of;
    const gck_uniform* shapes = cold->shapes;
    n_shapes = min(cold->n_shapes, (uint32_t)GCK_MAX_SHAPES);
    if ((uint32_t)lane < CPW && w0 + (uint32_t)lane < a.n) item_chunk.z = *(const GCK_GLOBAL uint8_t*)(shape_of + w0 + (uint32_t)lane);
    if ((uint32_t)lane < n_shapes) shape_ent = *(const GCK_GLOBAL u32x4*)(shapes + lane);
  }
  // the table in 16-B chunks (table_bytes is a multiple of 16, and at most TAB: the launch picks
  // the variant), every load issued before the first LDS write: one L2 round trip for the whole
  // table instead of one per pass of a word-by-word loop
  if (load_tab) {
    constexpr uint32_t kChunks = (TAB / 16u + kBlock - 1u) / kBlock;
    u32x4 tc[kChunks];
#pragma unroll
    for (uint32_t r = 0; r < kChunks; ++r) {
      const uint32_t at = (r * kBlock + threadIdx.x) * 16u;
      if (at < a.table_bytes && at < TAB) tc[r] = *(const GCK_GLOBAL u32x4*)(a.table + at);
    }
#pragma unroll
    for (uint32_t r = 0; r < kChunks; ++r) {
      const uint32_t at = (r * kBlock + threadIdx.x) * 16u;
      if (at < a.table_bytes && at < TAB) *reinterpret_cast<u32x4*>(&s_tab[at]) = tc[r];
    }
  }
  // (after the table's loads were issued: the entries' wait is the table's)
  if (__builtin_expect(shaped, 0) && (uint32_t)lane < n_shapes) *reinterpret_cast<u32x4*>(&s_item_w[lane * 4u]) = shape_ent;
  __syncthreads();
  if (__builtin_expect(grid, 0)) item_chunk.x = item_chunk.z, item_chunk.y = item_chunk.w;
  if (__builtin_expect(list, 0)) {  // (resource id, subject id): the varying id and the fixed one
    const bool sub = (a.mode & kCjListSub) != 0u;
    item_chunk.x = sub ? item_chunk.w : item_chunk.z;
    item_chunk.y = sub ? item_chunk.z : item_chunk.w;
  }
  const uint16_t* root = reinterpret_cast<const uint16_t*>(s_tab);
  const CjMeta* meta = reinterpret_cast<const CjMeta*>(s_tab + a.o_meta);
  const CjEntry* ent = reinterpret_cast<const CjEntry*>(s_tab + a.o_entries);
  const uint32_t i = (blk * kWaves + wib) * CPW + lane;
  const bool active = (uint32_t)lane < CPW && i < a.n && grid_on;
  const unsigned long long t_tab = timed ? wall_clock64() : 0ull;
  // (the task rounds below: row extents of what the slots left, then V(R), G(u), signatures, probes)
  bool take = false, self = false;
  uint32_t fast = 0;  // slot_decide: 2 HAS, 1 NO, 3 the list round, 0 the task rounds
  uint32_t l_cnt = 0;
  unsigned long long l_ptr = 0;
  uint32_t e = 0xFFFFu, nv = 0, ng = 0, vb = 0;
  unsigned long long gp = 0;
  // ---- round 0: the wave's items, one contiguous block -----------------------------------------
  if (uni) {
    // (the pairs are in registers)
  } else if (items_early) {
    // a full wave of 32: 40 chunks, lanes 0-39 (loaded above, beside the table)
    if (lane < 40) *reinterpret_cast<u32x4*>(&s_item_w[lane * 4u]) = item_chunk;
  } else if (CPW == 64 && ((uintptr_t)a.items & 15u) == 0 && item_bytes == 64u * 20u) {
    // a full wave: 80 chunks, lanes 0-15 take two; both loads in flight before either is stored
    const unsigned char* base = reinterpret_cast<const unsigned char*>(a.items) + (size_t)w0 * 20u;
    const u32x4 y0 = *(const GCK_GLOBAL u32x4*)(base + lane * 16u);
    const u32x4 y1 = lane < 16 ? *(const GCK_GLOBAL u32x4*)(base + (lane + 64u) * 16u) : u32x4{0u, 0u, 0u, 0u};
    *reinterpret_cast<u32x4*>(&s_item_w[lane * 4u]) = y0;
    if (lane < 16) *reinterpret_cast<u32x4*>(&s_item_w[(lane + 64u) * 4u]) = y1;
  } else if (((uintptr_t)a.items & 15u) == 0) {
    const unsigned char* base = reinterpret_cast<const unsigned char*>(a.items) + (size_t)w0 * 20u;
#pragma unroll
    for (uint32_t c = lane; c < CPW * 20u / 16u; c += 64u) {
      const uint32_t at = c * 16u;
      if (at + 16u <= item_bytes) {
        const u32x4 y = *(const GCK_GLOBAL u32x4*)(base + at);
        *reinterpret_cast<u32x4*>(&s_item_w[c * 4u]) = y;
      } else {
        for (uint32_t q = 0; q < 4u; ++q)  // the block's partial last chunk, by words
          if (at + 4u * q + 4u <= item_bytes) s_item_w[c * 4u + q] = gptr(reinterpret_cast<const uint32_t*>(base + at))[q];
      }
    }
  } else if (active) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.items + i);
    for (uint32_t q = 0; q < 5u; ++q) s_item_w[lane * 5u + q] = gptr(src)[q];
  }
  lds_wave_fence();
  const unsigned long long t_items = timed ? wall_clock64() : 0ull;
  gck_item it{};
  if (uni) {
    const auto cold = ax.cold();
    const uint32_t u_rp = cold->u_rp, u_ss = cold->u_ss, u_ctx = cold->u_ctx;
    if (__builtin_expect(shaped, 0)) {
      // (the wave's own LDS writes above are visible: the table's barrier lies between)
      const uint32_t sb = min(item_chunk.z, n_shapes - 1u);  // clamped before the lookup
      if (active) it = shaped_item(*reinterpret_cast<const u32x4*>(&s_item_w[sb * 4u]), item_chunk.z >= n_shapes, item_chunk.x, item_chunk.y);
    } else if (active) {
      it = uniform_item(u_rp, u_ss, u_ctx, item_chunk.x, item_chunk.y);
    }
  } else if (active) {
    uint32_t iw[5];
    for (uint32_t q = 0; q < 5u; ++q) iw[q] = s_item_w[lane * 5u + q];
    __builtin_memcpy(&it, iw, sizeof(it));
  }
  bool bad_w = false;
  if (a.mode & kCjBadSlot) {
    const auto cold = ax.cold();
    bad_w = check_slots(cold->bad_slot, cold->slot_limit, active, it, w0, lane);
  }
  // ---- round 1: both slots of every check the slots can take, line by line ---------------------
  unsigned long long ua = 0, da = 0, fa = 0, lbase = 0;  // (fa: the resource slot's front, half slots only)
  if (active && it.permission < a.n_fwd && it.subject_id != kWildcard && it.subject_relation == kEllipsis) {
    const uint32_t d = root[it.permission];
    if (d != 0xFFFFu && it.resource_type == meta[d].rtype && it.subject_type < a.n_types) {
      const CjEntry& E = ent[d * a.n_types + it.subject_type];
      if (E.uslot && E.dslot && it.subject_id < E.t_rows && it.resource_id < E.v_rows) {
        ua = (unsigned long long)(uintptr_t)(E.uslot + (size_t)it.subject_id * kUSlotWords);
        da = (unsigned long long)(uintptr_t)(E.dslot + (size_t)it.resource_id * kDSlotWords);
        lbase = (unsigned long long)(uintptr_t)E.ulist;
        if (HALF && E.dfront) fa = (unsigned long long)(uintptr_t)(E.dfront + (size_t)it.resource_id * kFrontWords);
      }
    }
  }
  // (the items are in registers now: the region takes the slot addresses)
  lds_wave_fence();
  s_ua[lane] = ua;
  s_da[lane] = da;
  const bool any_slots = __ballot(ua != 0) != 0;
  uint32_t dd[kDSlotWords];  // this lane's resource slot (the list round stages it again)
  uint32_t n_flag = 0;       // the wave's checks whose front said "read the slot" (timing builds record it)
  if (HALF && any_slots) {
    // the whole user slot (four lanes per 64-B line) and the first 32 B of the resource slot
    // (two lanes per half line) of every check: three loads per lane. The first half of a
    // resource slot holds up to 3 intervals — every document of config 4 (1-3 viewer groups) —
    // and a random 32-B read costs the memory system less than a 64-B one (tools/gather_probe:
    // 43.6 vs 25.6 G random reads/s); the lanes whose resource slot goes on read its second half
    // themselves below. (Half user slots too — users with <= 9 covers — measured slower: most
    // waves then had a lane with more covers, and so a second dependent round.)
    //
    // With fronts (CjEntry::dfront, 24-bit snapshots) the resource read is the check's own 16-B front
    // instead, one lane each, in the same round: four fronts share a 64-B line, so a quarter as many
    // lines carry the resources and more of the reads are Infinity Cache hits — which takes a
    // temporal load (tools/gather_probe --two-table: nontemporal, the layout changes nothing;
    // temporal, 16-B records read 2.9 % more checks/s than today's half slots). A flagged front
    // (slot_pack.hpp), or a check whose entry has none, reads its whole slot below.
    const bool fronts = __ballot(fa != 0) != 0;  // (wave-uniform: a scalar branch)
    u32x4 y[3];
#pragma unroll
    for (uint32_t r = 0; r < 2u; ++r) {  // user line of check 16 r + lane / 4, chunk lane % 4
      const unsigned long long b = s_ua[16u * r + ((uint32_t)lane >> 2)];
      y[r] = b ? slot_load((const GCK_GLOBAL u32x4*)(b + ((uint32_t)lane & 3u) * 16u)) : u32x4{0u, 0u, 0u, 0u};
    }
    if (fronts) {  // the check's own front (no front: flagged)
      y[2] = fa ? *(const GCK_GLOBAL u32x4*)fa : u32x4{kFrontReadSlot, kFrontReadSlot, kFrontReadSlot, kFrontReadSlot};
    } else {  // resource half line of check lane / 2, chunk lane % 2
      const unsigned long long b = s_da[(uint32_t)lane >> 1];
      y[2] = b ? slot_load((const GCK_GLOBAL u32x4*)(b + ((uint32_t)lane & 1u) * 16u)) : u32x4{0u, 0u, 0u, 0u};
    }
    lds_wave_fence();  // (the addresses are read)
#pragma unroll
    for (uint32_t r = 0; r < 2u; ++r) {
      const uint32_t chk = 16u * r + ((uint32_t)lane >> 2);
      *reinterpret_cast<u32x4*>(&s_slot_w[chk * kCheckWords + ((uint32_t)lane & 3u) * 4u]) = y[r];
    }
    if (!fronts)
      *reinterpret_cast<u32x4*>(&s_slot_w[((uint32_t)lane >> 1) * kCheckWords + kUSlotWords + ((uint32_t)lane & 1u) * 4u]) = y[2];
    lds_wave_fence();
    uint32_t w[kUSlotWords];
    if ((uint32_t)lane < CPW) {
      const uint32_t* src = &s_slot_w[(uint32_t)lane * kCheckWords];
#pragma unroll
      for (uint32_t q = 0; q < kUSlotWords; q += 4) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(&src[q]);
        w[q] = v.x, w[q + 1] = v.y, w[q + 2] = v.z, w[q + 3] = v.w;
      }
      if (!fronts) {
#pragma unroll
        for (uint32_t q = 0; q < 8u; q += 4) {
          const u32x4 v = *reinterpret_cast<const u32x4*>(&src[kUSlotWords + q]);
          dd[q] = v.x, dd[q + 1] = v.y, dd[q + 2] = v.z, dd[q + 3] = v.w;
        }
      }
    }
    // a flagged front's lane reads its slot itself (rare: the slots with more
    // than 3 intervals, long intervals, overflow slots); the others unpack theirs into the same words
    bool read_d = false;
    if (fronts) {
      const uint32_t f[kFrontWords] = {y[2].x, y[2].y, y[2].z, y[2].w};
      read_d = ua && (uint32_t)lane < CPW && front_flagged(f);
      front_unpack(f, dd);
      if (!ua || (uint32_t)lane >= CPW || read_d) {
#pragma unroll
        for (uint32_t q = 0; q < 8u; ++q) dd[q] = 0u;
      }
    }
#pragma unroll
    for (uint32_t q = 8; q < kDSlotWords; ++q) dd[q] = 0u;  // (empty intervals, as a fitting slot has them)
    n_flag = (uint32_t)__popcll(__ballot(read_d));
    if (__builtin_expect(n_flag != 0u, 0) && read_d) {  // (the whole slot: one round, not two)
#pragma unroll
      for (uint32_t q = 0; q < kDSlotWords; q += 4) {
        const u32x4 h = slot_load((const GCK_GLOBAL u32x4*)(da + 4u * q));
        dd[q] = h.x, dd[q + 1] = h.y, dd[q + 2] = h.z, dd[q + 3] = h.w;
      }
    }
    // second halves of the resource slots with more intervals (each lane its own check's)
    const bool more_d = ua && !read_d && !(dd[0] & kSlotOverflow) && dd[0] > kSlotHalfV;
    if (__builtin_expect(__ballot(more_d) != 0, 0) && more_d) {
      const u32x4 h0 = slot_load((const GCK_GLOBAL u32x4*)(da + 32u));
      const u32x4 h1 = slot_load((const GCK_GLOBAL u32x4*)(da + 48u));
      dd[8] = h0.x, dd[9] = h0.y, dd[10] = h0.z, dd[11] = h0.w;
      dd[12] = h1.x, dd[13] = h1.y, dd[14] = h1.z, dd[15] = h1.w;
    }
    uint32_t ng_l = 0, nv_l = 0;
    if (ua) {
      ng_l = slot_inline_count<BITS>(w[0]);
      nv_l = (dd[0] & kSlotOverflow) ? 0u : dd[0];
    }
    const uint32_t ng_max = wave_max(ng_l), nv_max = wave_max(nv_l);
    if (ua) {
      fast = slot_decide_wave<BITS>(w, dd, ng_max, nv_max);
      if (fast == 3u) {
        l_cnt = slot_list_count(w[0]);
        l_ptr = lbase + (unsigned long long)slot_list_off(w) * 4u;
        if (!lbase) fast = 0u;  // (no list array: the task rounds)
      }
    }
  } else if (any_slots) {
    lds_wave_fence();
    constexpr uint32_t kR = kSlotLines * 4 * CPW / 64;  // load instructions (16 lines each)
    u32x4 y[kR];
    unsigned long long bs[kR];
#pragma unroll
    for (uint32_t r = 0; r < kR; ++r) {  // line k = 16 r + lane / 4, chunk lane % 4
      const uint32_t k = 16u * r + ((uint32_t)lane >> 2), chk = k / kSlotLines, part = k - chk * kSlotLines;
      bs[r] = part == 0u ? s_ua[chk] : s_da[chk];
    }
#pragma unroll
    for (uint32_t r = 0; r < kR; ++r)  // (a check without slots has both addresses 0: nothing is read)
      y[r] = bs[r] ? slot_load((const GCK_GLOBAL u32x4*)(bs[r] + ((uint32_t)lane & 3u) * 16u)) : u32x4{0u, 0u, 0u, 0u};
    // every line is in flight; they are staged (and read back by their checks' lanes) half a wave
    // of checks at a time: instructions r < 4 carry checks 0-31, the others checks 32-63
    uint32_t w[kUSlotWords];
    constexpr uint32_t kRPer = kSlotLines * 4 / kStagePhases, kChkPer = 64 / kStagePhases;
    constexpr uint32_t kPh = kR / kRPer;  // phases with checks in them
#pragma unroll
    for (uint32_t ph = 0; ph < kPh; ++ph) {
      lds_wave_fence();  // the region's previous readers are done (addresses, or the last phase)
#pragma unroll
      for (uint32_t r = ph * kRPer; r < (ph + 1) * kRPer; ++r) {
        const uint32_t k = 16u * r + ((uint32_t)lane >> 2), chk = k / kSlotLines, part = k - chk * kSlotLines;
        *reinterpret_cast<u32x4*>(&s_slot_w[(chk - ph * kChkPer) * kCheckWords + part * 16u + ((uint32_t)lane & 3u) * 4u]) =
            y[r];
      }
      lds_wave_fence();
      if ((uint32_t)lane / kChkPer == ph) {
        const uint32_t* src = &s_slot_w[((uint32_t)lane - ph * kChkPer) * kCheckWords];
#pragma unroll
        for (uint32_t q = 0; q < kUSlotWords; q += 4) {
          const u32x4 v = *reinterpret_cast<const u32x4*>(&src[q]);
          w[q] = v.x, w[q + 1] = v.y, w[q + 2] = v.z, w[q + 3] = v.w;
        }
#pragma unroll
        for (uint32_t q = 0; q < kDSlotWords; q += 4) {
          const u32x4 v = *reinterpret_cast<const u32x4*>(&src[kUSlotWords + q]);
          dd[q] = v.x, dd[q + 1] = v.y, dd[q + 2] = v.z, dd[q + 3] = v.w;
        }
      }
    }
    // the wave's largest entry and interval counts bound the decision loops
    uint32_t ng_l = 0, nv_l = 0;
    if (ua) {
      ng_l = slot_inline_count<BITS>(w[0]);
      nv_l = (dd[0] & kSlotOverflow) ? 0u : dd[0];
    }
    const uint32_t ng_max = wave_max(ng_l), nv_max = wave_max(nv_l);
    if (ua) {
      fast = slot_decide_wave<BITS>(w, dd, ng_max, nv_max);
      if (fast == 3u) {
        l_cnt = slot_list_count(w[0]);
        l_ptr = lbase + (unsigned long long)slot_list_off(w) * 4u;
        if (!lbase) fast = 0u;  // (no list array: the task rounds)
      }
    }
  }
  const unsigned long long t_slot1 = timed ? wall_clock64() : 0ull;
  // (timing builds: the wave's checks that go into round 1b; the bits above n_take in its word)
  const uint32_t n_list = timed ? (uint32_t)__popcll(__ballot(fast == 3u)) : 0u;
  // ---- round 1b: the cover lists of users whose covers exceed a slot, one (check, entry) task
  // per lane slot, against the check's intervals staged in LDS ------------------------------------
  if (__builtin_expect(__ballot(fast == 3u) != 0, 0)) {
    // the resource slots of the list checks, one per lane, for the (check, entry) tasks below
    lds_wave_fence();
    if (fast == 3u) {
#pragma unroll
      for (uint32_t q = 0; q < kDSlotWords; q += 4)
        *reinterpret_cast<u32x4*>(&s_slot_w[lane * kDSlotWords + q]) = u32x4{dd[q], dd[q + 1], dd[q + 2], dd[q + 3]};
    }
    const uint32_t nl = fast == 3u ? l_cnt : 0u;
    s_gp[wib][lane] = l_ptr;
    s_hit[wib][lane] = 0u;
    const uint32_t lincl = wave_incl_scan(nl);
    const uint32_t ltotal = wave_last(lincl);
    s_excl[wib][lane] = lincl - nl;
    if (lane == 63) s_excl[wib][64] = ltotal;
    lds_wave_fence();
    for (uint32_t t0 = 0; t0 < ltotal; t0 += 64u * kCjL) {
      uint32_t x[kCjL], own[kCjL];
#pragma unroll
      for (int u = 0; u < kCjL; ++u) {  // all loads in flight together
        const uint32_t t = t0 + u * 64u + lane;
        own[u] = 0xFFFFFFFFu;
        x[u] = 0u;
        if (t < ltotal) {
          const uint32_t o = owner_of(s_excl[wib], t);
          own[u] = o;
          x[u] = *(const GCK_GLOBAL uint32_t*)(s_gp[wib][o] + 4ull * (t - s_excl[wib][o]));
        }
      }
#pragma unroll
      for (int u = 0; u < kCjL; ++u) {
        if (own[u] == 0xFFFFFFFFu) continue;
        const uint32_t* dv = &s_slot_w[own[u] * kDSlotWords];
        const uint32_t nv = dv[0];
        bool hit = false;
#pragma unroll
        for (int j = 0; j < kSlotV; ++j) hit |= (uint32_t)j < nv && dv[2 + 2 * j] <= x[u] && x[u] < dv[3 + 2 * j];
        if (hit) atomicOr(&s_hit[wib][own[u]], 1u);
      }
    }
    lds_wave_fence();
    if (fast == 3u) fast = lds_ld(&s_hit[wib][lane]) ? 2u : 1u;
  }
  const unsigned long long t_slots = timed ? wall_clock64() : 0ull;
  // Everything from here to the results is for checks the slots did not decide. A wave without
  // one (every wave of config 4) skips it whole — the set-up stores, the scan and the fences as
  // well as the loops — and the branch is marked unlikely, as the other rare ones are, so that the
  // compiler lays the slot path out as straight-line code with the rare rounds behind it: a
  // skipped round in the middle of the path cost the waves of a batch, which start together after
  // the dispatch has invalidated the instruction cache, a miss each. (The 1.2 us the timing build
  // showed between the slot decisions and the extents was the list round itself: more than half of
  // the flagship's waves held a listed check until listed slots carried inline entries and a window.)
  uint32_t total = 0, probes = 0;
  unsigned long long t_r1 = t_slots;
  if (__builtin_expect(__ballot(active && !fast) != 0, 0)) {
  // ---- the task rounds' inputs for the rest: row extents ----------------------------------------
  if (active && !fast) {
    if (it.permission < a.n_fwd && it.subject_id != kWildcard) {
      const uint32_t d = root[it.permission];
      if (d != 0xFFFFu && it.resource_type == meta[d].rtype && it.subject_type < a.n_types) {
        const CjMeta M = meta[d];
        e = d * a.n_types + it.subject_type;
        const CjEntry& E = ent[e];
        if (it.subject_relation == kEllipsis) {
          if (E.t_off && it.subject_id < E.t_rows) {
            const uint32_t b = gptr(E.t_off)[it.subject_id], en = gptr(E.t_off)[it.subject_id + 1];
            ng = en - b;
            gp = (unsigned long long)(uintptr_t)(E.t_nbr + b);
            take = true;
          }
        } else if (it.subject_relation == M.mrel && it.subject_type == M.mtype && it.subject_id < M.m_rows) {
          ng = 1;
          gp = it.subject_id;
          self = true;
          take = true;
        }
        if (take) {
          if (E.v_off) {
            take = it.resource_id < E.v_rows;
            if (take) {
              vb = gptr(E.v_off)[it.resource_id];
              nv = gptr(E.v_off)[it.resource_id + 1] - vb;
            }
          } else {
            take = it.resource_id < M.m_rows;
            nv = 1;
            vb = it.resource_id;
          }
        }
        if (take && (nv > (uint32_t)kCjV || ng > kCjG)) take = false;  // left to the bundle stages
      }
    }
  }
  // ---- round 2: the (check, g) tasks over the wave; V(R) loads issued with the first groups ----
  const uint32_t nt = (take && nv) ? ng : 0u;  // an empty V(R) is NO: no tasks
  s_nv[wib][lane] = nv | (self ? 0x80000000u : 0u);
  s_e[wib][lane] = (uint16_t)e;
  s_gp[wib][lane] = gp;
  s_hit[wib][lane] = 0u;
  const uint32_t incl = wave_incl_scan(nt);
  total = wave_last(incl);
  t_r1 = timed ? wall_clock64() : 0ull;
  uint32_t* excl = s_excl[wib];
  excl[lane] = incl - nt;
  if (lane == 63) excl[64] = total;
  lds_wave_fence();
  uint32_t vv[kCjV];
  const uint32_t* vsrc = (take && ent[e].v_off) ? ent[e].v_nbr + vb : nullptr;
#pragma unroll
  for (int k = 0; k < kCjV; ++k) vv[k] = (vsrc && (uint32_t)k < nv) ? gptr(vsrc)[k] : 0u;
  bool v_stored = false;
  for (uint32_t t0 = 0; t0 < total; t0 += 64u * kCjK) {
    uint32_t g[kCjK], own[kCjK];
#pragma unroll
    for (int u = 0; u < kCjK; ++u) {  // the tasks' groups, all loads in flight together
      const uint32_t t = t0 + u * 64u + lane;
      g[u] = kNone;
      own[u] = 0;
      if (t < total) {
        const uint32_t o = owner_of(excl, t);
        own[u] = o;
        const unsigned long long b = s_gp[wib][o];
        g[u] = (s_nv[wib][o] & 0x80000000u) ? (uint32_t)b
                                             : gptr(reinterpret_cast<const uint32_t*>(b))[t - excl[o]];
      }
    }
    if (!v_stored) {  // V(R) (loaded together with the first groups) into LDS for the tests
      v_stored = true;
      if (take) {
        if (vsrc) {
#pragma unroll
          for (int k = 0; k < kCjV; ++k)
            if ((uint32_t)k < nv) s_v_w[lane][k] = vv[k];
        } else {
          s_v_w[lane][0] = vb;
        }
      }
      lds_wave_fence();
    }
    uint32_t sg[kCjK][kSigWords];
#pragma unroll
    for (int u = 0; u < kCjK; ++u) {  // their signatures, all in flight together
      // (a group past the closure's rows — added by a Watch batch without nesting — has no
      // ancestors and no signature: only g == v can hit)
      if (g[u] != kNone && g[u] < meta[s_e[wib][own[u]] / a.n_types].m_rows) {
        const GCK_GLOBAL u64x2* q = (const GCK_GLOBAL u64x2*)(ent[s_e[wib][own[u]]].sig + (size_t)g[u] * kSigWords);
        const u64x2 x0 = q[0], x1 = q[1];
        sg[u][0] = (uint32_t)x0.x, sg[u][1] = (uint32_t)(x0.x >> 32), sg[u][2] = (uint32_t)x0.y;
        sg[u][3] = (uint32_t)(x0.y >> 32), sg[u][4] = (uint32_t)x1.x, sg[u][5] = (uint32_t)(x1.x >> 32);
        sg[u][6] = (uint32_t)x1.y, sg[u][7] = (uint32_t)(x1.y >> 32);
      } else {
#pragma unroll
        for (uint32_t k = 0; k < kSigWords; ++k) sg[u][k] = 0u;
      }
    }
#pragma unroll
    for (int u = 0; u < kCjK; ++u) {  // g in V(R), or a signature hit the closure index confirms
      if (g[u] == kNone) continue;
      const uint32_t o = own[u];
      if (lds_ld(&s_hit[wib][o])) continue;
      const uint32_t n_v = s_nv[wib][o] & 0x7FFFFFFFu;
      bool hit = false;
      for (uint32_t k = 0; k < n_v && !hit; ++k) {
        const uint32_t v = s_v_w[o][k];
        if (v == g[u]) {
          hit = true;
        } else if (sig_has(sg[u], v)) {
          const CjEntry& E = ent[s_e[wib][o]];
          const unsigned long long key = mkey(g[u], v);
          const uint32_t bk = (uint32_t)(mix64(key) & E.anc_bmask);
          ++probes;
          DevCSR r{};
          r.mhash = E.anc_hash;
          r.mmask = E.anc_bmask;
          hit = mhash_finish(r, bk, key, bucket_probe(E.anc_hash, bk, key), probes);
        }
      }
      if (hit) atomicOr(&s_hit[wib][o], 1u);
    }
  }
  lds_wave_fence();
  }
  const unsigned long long t_tasks = timed ? wall_clock64() : 0ull;
  // the batch counters: summed per block in LDS, one atomic per block and counter (an atomic per
  // wave on the same line serialises at the L2 behind every other wave's). Only probes and the
  // task-round checks are counted here — both zero on the slot path, so a block of slot checks
  // issues no atomic; the host derives the rest from the deferred count.
  __shared__ unsigned s_cnt[4];  // probes, task-round checks, deferred checks, a bad context slot
  if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  if (lane == 0 && bad_w) atomicOr(&s_cnt[3], 1u);
  uint32_t wprobes = probes;
  for (int o = 32; o > 0; o >>= 1) wprobes += __shfl_xor(wprobes, o, 64);
  if (lane == 0 && wprobes) atomicAdd(&s_cnt[0], wprobes);
  if (uni) {
    const uint32_t v = (active && fast) ? (fast == 2u ? (uint32_t)GCK_PERM_HAS : (uint32_t)GCK_PERM_NO)
                       : (active && take) ? (lds_ld(&s_hit[wib][lane]) ? (uint32_t)GCK_PERM_HAS : (uint32_t)GCK_PERM_NO)
                                          : 0u;
    packed_store(ax.cold()->out_packed, w0, v, lane, CPW, a.n);
  } else if (active && fast) {
    store_result(a.out_perm + i, fast == 2u ? (uint8_t)GCK_PERM_HAS : (uint8_t)GCK_PERM_NO, (a.mode & kPubCoherent) != 0u);
    store_result(a.out_err + i, (int32_t)GCK_ITEM_OK, (a.mode & kPubCoherent) != 0u);
  } else if (active && take) {
    store_result(a.out_perm + i, lds_ld(&s_hit[wib][lane]) ? (uint8_t)GCK_PERM_HAS : (uint8_t)GCK_PERM_NO,
                 (a.mode & kPubCoherent) != 0u);
    store_result(a.out_err + i, (int32_t)GCK_ITEM_OK, (a.mode & kPubCoherent) != 0u);
  }
  {  // checks left to the bundles: one counter add per wave (labels.inc wave_append)
    const bool left = active && !fast && !take;
    const unsigned long long m = __ballot(left);
    if (__builtin_expect(m != 0, 0)) {
      const int leader = __ffsll((long long)m) - 1;
      const auto cold = ax.cold();
      uint32_t base = 0;
      if (lane == leader) {
        base = atomicAdd(cold->n_deferred, (unsigned)__popcll(m));
        atomicAdd(&s_cnt[2], (unsigned)__popcll(m));
      }
      base = (uint32_t)__shfl((int)base, leader, 64);
      if (left) cold->deferred[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
      if (left && uni) {  // the check's item where the bundle stages read it (its pair read again: rare)
        if (a.mode & kCjGrid) {  // (a cross batch: its two ids by (row, column))
          uint32_t res, sub;
          cross_ids_again(cold->pairs, cold->cols, i, res, sub);
          cold->items_out[i] = uniform_item(cold->u_rp, cold->u_ss, cold->u_ctx, res, sub);
        } else if (list) {  // (a list batch: its varying id again, the fixed one beside it)
          uint32_t res, sub;
          list_ids_again(cold->pairs, a.mode >> kCjListShift, cold->cols, cold->u_fixed, i, res, sub);
          cold->items_out[i] = uniform_item(cold->u_rp, cold->u_ss, cold->u_ctx, res, sub);
        } else {
          const unsigned long long pr = *(const GCK_GLOBAL unsigned long long*)(cold->pairs + 2ull * i);
          if (shaped)
            cold->items_out[i] = shaped_item_again(cold->shape_of, cold->shapes, n_shapes, i, (uint32_t)pr, (uint32_t)(pr >> 32));
          else
            cold->items_out[i] = uniform_item(cold->u_rp, cold->u_ss, cold->u_ctx, (uint32_t)pr, (uint32_t)(pr >> 32));
        }
      }
    }
  }
  const uint32_t n_take = (uint32_t)__popcll(__ballot(active && (take || fast)));
  const uint32_t n_task = (uint32_t)__popcll(__ballot(active && take && !fast));
  if (lane == 0 && n_task) atomicAdd(&s_cnt[1], n_task);
  if ((a.mode & kCjSelfPub) && (a.mode & kPubCoherent)) __builtin_amdgcn_s_waitcnt(0);  // (coherent results: completed before the block arrives)
  __syncthreads();
  const uint32_t blk_deferred = s_cnt[2];
  if (threadIdx.x == 0 && (s_cnt[0] | s_cnt[1])) {
    DevCounters* ctr = ax.ctr();
    if (s_cnt[0]) atomicAdd(&ctr->probes, (unsigned long long)s_cnt[0]);
    if (s_cnt[1]) atomicAdd(&ctr->closure, (unsigned long long)s_cnt[1]);
  }
  if (a.mode & kPubBySignal) {
    if (threadIdx.x == 0) block_summary_cold(ax, s_cnt[2], s_cnt[0] | s_cnt[1] | s_cnt[3], blk);
  } else if ((a.mode & kCjSelfPub) && wib == 0) {
    const auto cold = ax.cold();
    // the batch's publication without a k_publish launch (one host launch per batch instead of
    // two: the host submit cost bounds the batches in flight), by wave 0 of each block after the
    // block's barrier (the other waves are done). The counters are device-scope atomics,
    // coherent by themselves: a block arrives (an atomic on `done`) once its own have completed
    // (s_waitcnt: no release fence, which would write back and invalidate the L2 in every
    // block); the last to arrive reads and zeroes the counters with atomics, writes them to
    // coherent host memory and releases the sequence word the host spins on. (The deferred list
    // is stream-ordered: read by later launches on this stream. The results are too on a caller's
    // stream; on an engine stream they are agent-scope stores, `coherent`, that every wave has
    // waited for before the barrier.)
    uint32_t last = 0;
    if (lane == 0) {
      __builtin_amdgcn_s_waitcnt(0);  // this thread's counter atomics have completed
      last = atomicAdd(cold->done, 1u) == ax.nblk() - 1u;
    }
    if (__shfl(last, 0, 64)) {
      unsigned* h_out = cold->h_out;
      unsigned* pub = cold->pub;
      const uint32_t pub_words = cold->pub_words;
      for (uint32_t k = lane; k < pub_words; k += 64u) h_out[k] = atomicExch(&pub[k], 0u);
      if (lane == 0) pub_seq_store(h_out + pub_words, cold->seq, a.mode);
    }
  }
  if (timed) {
    const uint32_t wave_probes = wave_last(wave_incl_scan(probes));
    if (lane == 0) {
      unsigned long long* t = ax.cold()->timing + (unsigned long long)kCjTimingWords * (blk * kWaves + wib);
      t[0] = t_start;
      t[1] = t_tab;
      t[2] = t_r1;
      t[3] = t_tasks;
      t[4] = wall_clock64();
      t[5] = total;
      t[6] = wave_probes;
      t[7] = n_take | (unsigned long long)n_list << 32;
      t[8] = t_items;
      t[9] = t_slots;
      t[10] = t_slot1;
      t[11] = n_flag;
    }
  }
  return blk_deferred;
}

template <int BITS, uint32_t TAB, uint32_t CPW = 64, bool HALF = false>
__global__ void __launch_bounds__(kBlock) k_closure_join(Ctx c, CjArgs a) {
  // (c and a are read through the kernarg segment: CjKernargs)
  const unsigned long long t_start = GCK_BUNDLE_TIMING ? wall_clock64() : 0ull;
  CjKernargs ax;
  ax.load_hot();
  cj_block<BITS, TAB, CPW, HALF>(ax, blockIdx.x, true, t_start);
}

// The closure join's variants: the kernel a HIP launch takes and, for the one the engine also
// dispatches into its HSA queues (aql.inc), its demangled name in libgck_kernels.co — side by side,
// so that the two cannot name different kernels.
struct CjVariant {
  void (*kernel)(Ctx, CjArgs);
  const char* aql_name;  // null: launched through HIP only
  uint32_t cpw;          // checks per wave
};

static const CjVariant& cj_variant(uint32_t slot_bits, bool small);  // (engine.hip, beside the join's launch)
