// labels.inc — the label join: a one-round check for union / intersection / exclusion permissions
// over nested usersets and arrow chains (included by engine.hip after bidir.inc).
//
// The closure join (closure.inc) answers one shape, doc#view = group#member nested groups. Most
// schemas are wider: BASELINE config 2 (Google Docs) reaches a document's grants through a chain
// of parent folders (`parent->view`) and grants to direct users and to nested groups; config 3
// (GitHub) grants through teams nested in teams, through an organisation's members
// (`org->is_member`), and combines them with exclusion (`- banned`) and intersection (`&`).
// SpiceDB answers such a check by walking the rewrite tree (client/client.go:262 CheckBulkPermissions;
// SURVEY §5.1). Below the depth budget, without caveats and expirations, that walk is a
// reachability question per operand — HAS iff the subject is reached — so the check splits into a
// resource side and a subject side that meet at *hubs*:
//
//   hub        a node that usersets or arrows point at and that is itself only a union of stored
//              subjects and usersets of hubs (`group#member`, `team#member`, `org#is_member`);
//              its objects are the vertices of one hierarchy (x -> y when x lists y#h');
//   subject    the hub vertices that list user u directly, closed upwards in the hierarchy:
//              A(u). Stored as tree covers in a 64-B user slot (closure.inc, k_user_slots_1p): v is
//              in A(u) iff some cover entry of u lies in v's preorder interval [pre(v), end(v));
//   resource   per (permission p, resource R) and per operand ("term") of p: the users D the
//              operand reaches without entering a hub, the hub vertices V where it enters one
//              (their intervals), and whether a wildcard reaches it — flattened once, through any
//              arrow chain (the folder forest), into a resource slot.
//
// A check (R, p, u) reads its user slot and its resource slot — lines fetched by the whole wave,
// all in flight together — and decides each term: hit = wildcard | u in D | a cover in a V
// interval; the permission is the conjunction of its terms, each possibly negated (`-` operands).
// Exact: no signature, no probe, one round of memory. Checks whose slots do not fit (long cover
// lists, large flattened sets) take a second, per-lane round over lists; what the slots cannot
// answer (a resource at or above the depth budget, an overflowing hierarchy vertex, another subject
// type, a userset subject) goes to the wave bundles (bundle.inc) on the device.

constexpr uint32_t kLjHdrOverflow = 0x80000000u;  // resource slot: not answerable here (deferred)
constexpr uint32_t kLjHdrExt = 0x40000000u;       // resource slot: the record is in the extension array (w[1])
// resource slot of a root with at most two terms (the third term's field is free) or an extension
// record: a Watch batch changed a wildcard grant the root reads on the resource's own object — the
// slot's wildcard bits and wildcard pairs are stale, the rest holds (the chain walk decides it)
constexpr uint32_t kLjHdrWildDirty = 0x20000000u;
constexpr int kLjTerms = 3;                       // operands of a permission (terms)
constexpr uint32_t kLjMaxD = 31, kLjMaxV = 15;    // per term, in an inline slot (5 + 4 bits)
constexpr uint32_t kLjLdsBytes = 2048;            // the root table, staged in LDS
constexpr uint32_t kLjFlatCap = 4096;             // per flattened term: visited vertices, D, V
constexpr uint32_t kLjCoverMax = 64;              // cover entries per hierarchy vertex (more: it overflows)
constexpr uint32_t kLjDeep = 0x80000000u;         // lab[2v + 1] of a hub root's vertex at the depth budget
// A caveated root (LjMeta::cav) may list, after a term's plain users, users reached through a
// caveated relationship as word pairs (kLjCav | user, caveat instance); a caveated wildcard is the
// user kLjCavWild. Plain users are < 2^31 (interned ids), so a pair never equals a plain entry.
constexpr uint32_t kLjCav = 0x80000000u;
constexpr uint32_t kLjCavWild = 0x7FFFFFFFu;
// Per dirty subject (LjTables::dov), two lines: word 0 the appends made (low 31 bits) |
// kDovOver once one did not fit, word 1 unused, then kDovPairs (lo, hi) arrow-forest intervals of
// the objects whose direct grants of the subject changed since the tables were built — pairs 0-6
// in the first line, 7-14 in the second.
constexpr uint32_t kDovWords = 32, kDovPairs = 15, kDovOver = 0x80000000u;

// The chain program of a root (labels_build.inc lj_chain_of): per term, the direct-user CSR classes its
// flattening reads at each depth of the resource's arrow-forest chain (R, R's parent, ...), so that a
// dirty subject's check whose overlay hits (a changed grant on the chain) is decided in the join
// from the current revision's rows instead of going to the bundles. A level is one set of schema
// nodes on one object; the levels of a term form a path that may loop (a folder's parent->view
// reaches folder#view again).
constexpr uint32_t kLjChainCls = 8, kLjChainLvls = 8, kLjChainDepth = 64;
constexpr uint8_t kLjChainEnd = 0xFF;
struct LjChainLvl {
  uint32_t af_base;             // forest index of object 0 of the level's type (LjTables::af_base)
  uint16_t csr[kLjChainCls];    // direct-user classes (plain or caveated) read on the level's object
  uint16_t arrow;               // the tupleset CSR whose row leads to the next depth (0xFFFF: none)
  uint8_t n, next;              // classes; the next depth's level (kLjChainEnd: the term's walk ends)
};
struct LjChain {
  uint8_t first[4];             // per term its depth-0 level (kLjChainEnd: no program)
  LjChainLvl lvl[kLjChainLvls];
};
static_assert(sizeof(LjChainLvl) == 24, "LjChainLvl layout");

struct LjMeta {  // one label root (a permission) and its subject type
  const uint32_t* uslot;  // kUSlotWords per subject (closure.inc user slots over the hub hierarchy)
  const uint32_t* ulist;  // cover lists of subjects whose covers exceed a slot (null: none)
  const uint32_t* rslot;  // sw words per resource
  const uint32_t* rext;   // extension records (null: none)
  uint32_t u_rows, r_rows;
  uint16_t rtype, utype;
  uint8_t n_terms, neg;  // neg bit t: term t is subtracted (exclusion operand)
  uint8_t cav;           // the terms may hold caveated pairs (kLjCav)
  uint8_t pack;          // inline slots hold 24-bit fields (LjEnt24), not 32-bit words
  // the resources' (pre, end) in the arrow forest (LjTables::af; null: none): a dirty
  // subject's check stays with the slots unless a changed object's interval holds pre(R)
  const uint32_t* apre;
  // the chain program (null: a dirty subject's overlay hit defers the check)
  const LjChain* chain;
};
static_assert(sizeof(LjMeta) == 64, "LjMeta layout");

struct LjArgs {
  const gck_item* items;
  uint32_t n;
  uint32_t list;  // a list batch (closure.inc CjArgs::list: kListOn | kListSubject | kListRange); 0 otherwise
  uint8_t* out_perm;
  int32_t* out_err;
  uint32_t* deferred;          // checks left to the bundle stages
  unsigned* n_deferred;
  const unsigned char* table;  // root[n_fwd] u16 (0xFFFF: not a label root), then LjMeta[]
  uint32_t n_fwd, table_bytes, o_meta;
  // publication of a device batch on the caller's stream (as CjArgs; null h_out: k_publish follows)
  unsigned* pub;
  unsigned* h_out;
  unsigned* done;
  uint32_t pub_words, seq;
  uint32_t coherent;  // results written through the L2 (engine-stream batches published by the join)
  uint32_t u_fixed;   // a list batch: the fixed id (closure.inc CjArgs::u_fixed)
  // the call's check contexts (a device copy of the batch's Ctx: caveat outcomes, the lazy
  // evaluation's request set, cav_flag), or null: a caveated pair is then CONDITIONAL
  const Ctx* cx;
  // subjects whose direct grants changed since the tables were built (a bit each; null: none):
  // their checks go to the bundles (labels_build.inc lj_dirty_path)
  const uint32_t* dirty;
  // the caveat instances and the dense outcome table's rows (k_label_join<..., CL>: staged in LDS)
  uint32_t cav_n, cav_rows;
  // host items read in place: the request check of their context slots (CjArgs::bad_slot)
  unsigned* bad_slot;
  uint32_t slot_limit;
  uint32_t n_shapes;  // a shaped batch (below): the table's entries; 0: not shaped
  // the dirty subjects' changed objects (kDovWords per subject; null: a dirty subject defers)
  const uint32_t* dov;
  unsigned long long* timing;  // GCK_DEBUG_TIMING (TIMING=1 builds): kLjTimingWords per wave
  // a uniform batch (closure.inc CjArgs::pairs)
  const uint32_t* pairs;
  unsigned long long* out_packed;
  gck_item* items_out;
  // ... or a shaped batch (closure.inc CjArgs::shapes; n_shapes != 0, with `pairs`): the index bytes
  // and the table lie over the header words, which it does not use
  union {
    struct {
      uint32_t u_rp, u_ss, u_ctx;
      // a cross batch (closure.inc CjArgs::cols) when n_shapes == 0 and list == 0; a list batch's
      // range: its first id; else 0 or part of `shapes`
      uint32_t cols;
    };
    struct {
      const uint8_t* shape_of;
      const gck_uniform* shapes;
    };
  };
  // the chain walk of a dirty subject's overlay hit (LjMeta::chain): the current revision's CSRs
  // and the forest's parent edges (LjTables::afp: tupleset CSR << 32 | parent's index)
  const DevCSR* csrs;
  const unsigned long long* afp;
  uint32_t n_csrs, afp_n;  // (the walk's bounds: every index it reads is checked against them)
  const uint8_t* cav_static;  // per caveat instance its outcome under its stored context (the walk)
  const uint32_t* anc;        // per forest vertex its ancestors (kAncWords, LjTables::anc; null: none)
};
// per wave: {start, items and table staged, slot lines staged, decided, end, list checks, ext checks,
// deferred: no label root / a slot overflow / a dirty subject without the overlay / an overlay hit}
constexpr int kLjTimingWords = 11;  // (+ deferred checks by reason: no root, slot overflow, dirty subject, dirty hit)

// Caveat tables small enough to stage in LDS for a batch with check contexts (the dense outcome
// table of gck_api.cpp caveat_call): a caveated pair is then decided without a global round.
constexpr uint32_t kLjCavInst = 512, kLjCavDense = 4096, kLjCavCtx = 512;
struct LjCavLds {
  uint8_t st[kLjCavInst];     // Ctx::cav_static
  uint16_t row[kLjCavInst];   // Ctx::cav_row (0xFFFF: none)
  uint8_t dyn[kLjCavDense];   // Ctx::cav_dyn, rows x n_dist
  uint8_t slot[kLjCavCtx];    // Ctx::cav_slot
};
struct LjNoCavLds {};

// A slot in a list whose length is *counter for every lane with `pred`, one atomic per wave (a
// per-lane add to one counter serialises every lane of the batch at the L2). All lanes call it.
__device__ __forceinline__ uint32_t wave_append(unsigned* counter, bool pred) {
  const unsigned long long m = __ballot(pred);
  if (!m) return 0u;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)m) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(counter, (unsigned)__popcll(m));
  base = (uint32_t)__shfl((int)base, leader, 64);
  return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// The entries of a resource record: 32-bit words (extension records; inline slots of a snapshot
// whose ids need more than 24 bits), or 24-bit fields packed from bit 32 of an inline slot (its
// header is word 0): a config-2 document's flattened users and intervals then fit one line more
// often. A caveated pair's user carries kCav; a caveated wildcard is kWild.
struct LjEnt32 {
  const uint32_t* p;
  static constexpr uint32_t kCav = kLjCav, kWild = kLjCavWild;
  __device__ __forceinline__ uint32_t operator[](uint32_t k) const { return p[k]; }
  __device__ __forceinline__ LjEnt32 skip(uint32_t k) const { return {p + k}; }
};
struct LjEnt24 {
  const uint32_t* w;  // the slot (word 0: the header)
  uint32_t f0;        // the first field of these entries
  static constexpr uint32_t kCav = 0x800000u, kWild = 0x7FFFFFu;
  __device__ __forceinline__ uint32_t operator[](uint32_t k) const {
    const uint32_t b = 32u + 24u * (f0 + k), i = b >> 5, sh = b & 31u;
    uint32_t v = w[i] >> sh;
    if (sh > 8u) v |= w[i + 1] << (32u - sh);
    return v & 0xFFFFFFu;
  }
  __device__ __forceinline__ LjEnt24 skip(uint32_t k) const { return {w, f0 + k}; }
};

// One term over a record's entries: wildcard, u among the nD users, or a cover among the nV
// intervals (lo, len): lo <= c < lo + len iff c - lo < len. The entries may lie in LDS or HBM.
// CAV: the users may end with caveated pairs, whose caveat (`cavf`: 0 false, 1 true, 2 unresolved)
// decides them. 2 reached, 1 not, 3 reached only through unresolved caveats.
template <bool CAV, class Ent, class Covers, class CavF>
__device__ __forceinline__ uint32_t lj_term(uint32_t u, bool wild, uint32_t nD, uint32_t nV, const Ent& ent,
                                            const Covers& cov, const CavF& cavf, uint32_t kwild = Ent::kWild) {
  // (kwild: the caveated wildcard's id, or kLjNoUser when the slot's wildcard entries are stale)
  bool hit = wild, cond = false;
  if (CAV) {
    // every caveated relationship of the subject on the walk is evaluated, as SpiceDB's dispatch
    // evaluates each one it meets (a failing one fails the check, whatever else holds)
    for (uint32_t k = 0; k < nD; ++k) {
      const uint32_t w = ent[k];
      if (w & Ent::kCav) {
        const uint32_t x = w & ~Ent::kCav;
        if (x == u || x == kwild) {
          const uint32_t s = cavf(ent[k + 1]);
          hit |= s == 1u;
          cond |= s == 2u;
        }
        ++k;
      } else {
        hit |= w == u;
      }
    }
  } else {
    // (no early exit: the entry reads do not wait for one another, so they pipeline — with a
    // 24-bit field two LDS words each)
#pragma unroll 4
    for (uint32_t k = 0; k < nD; ++k) hit |= ent[k] == u;
  }
  for (uint32_t j = 0; j < nV && !hit; ++j) hit = cov.any_in(ent[nD + 2 * j], ent[nD + 2 * j + 1]);
  return hit ? 2u : cond ? 3u : 1u;
}

template <int BITS>
struct LjInlineCovers {  // the covers of an inline user slot, unpacked
  uint32_t p[kSlotGMax];
  uint32_t ng;
  __device__ __forceinline__ bool any_in(uint32_t lo, uint32_t len) const {
    bool hit = false;
#pragma unroll
    for (int k = 0; k < slot_cap<BITS>(); ++k) hit |= (uint32_t)k < ng && p[k] - lo < len;
    return hit;
  }
};

struct LjListCovers {  // a cover list in HBM (32-bit preorder numbers)
  const uint32_t* list;
  uint32_t ng;
  __device__ __forceinline__ bool any_in(uint32_t lo, uint32_t len) const {
    for (uint32_t k = 0; k < ng; ++k)
      if (gptr(list)[k] - lo < len) return true;
    return false;
  }
};

// The permission over a resource record: inline (the slot `rw`, header rw[0]; 24-bit fields when
// P24) or an extension record (rec: [n_terms | wild bits << 8], then (nD, nV) per term, then the
// entries as words). The conjunction of the terms, each possibly negated, in SpiceDB's tri-state
// algebra (intersection and exclusion: any NO is NO, else any CONDITIONAL is CONDITIONAL):
// GCK_PERM_HAS / NO / CONDITIONAL.
// A term's outcome (2 reached, 3 reached only through unresolved caveats, 1 not) joined with another.
__device__ __forceinline__ uint32_t lj_tri_or(uint32_t a, uint32_t b) {
  return (a == 2u || b == 2u) ? 2u : (a == 3u || b == 3u) ? 3u : 1u;
}

// WALK: the subject's own entries are not in the slot's answer (u is kLjNoUser, which no entry
// equals) and `walk` holds, 2 bits per term, what lj_chain_walk found for it on the current rows.
constexpr uint32_t kLjNoUser = 0xFFFFFFFFu;
template <bool CAV, bool P24, bool WALK = false, class Covers, class CavF>
__device__ __forceinline__ uint32_t lj_decide(uint32_t u, uint32_t hdr, const uint32_t* rw, const uint32_t* rec,
                                              uint32_t n_terms, uint32_t neg, const Covers& cov, const CavF& cavf,
                                              uint32_t walk = 0u, bool xw = false) {
  // (xw, WALK only: the slot's wildcard bits and wildcard pairs are left out — the walk read them)
  bool no = false, cond = false;
  auto fold = [&](uint32_t v, uint32_t t) {
    if (WALK) v = lj_tri_or(v, (walk >> (2u * t)) & 3u);
    if ((neg >> t) & 1u) v = v == 2u ? 1u : v == 1u ? 2u : v;
    no |= v == 1u;
    cond |= v == 3u;
  };
  if (!(hdr & kLjHdrExt)) {
    auto ent = [&] {
      if constexpr (P24) return LjEnt24{rw, 0u};
      else return LjEnt32{rw + 1};
    }();
    for (uint32_t t = 0; t < n_terms; ++t) {
      const uint32_t f = hdr >> (10u * t);
      const uint32_t nD = f & 31u, nV = (f >> 5) & 15u;
      fold(lj_term<CAV>(u, !(WALK && xw) && ((f >> 9) & 1u), nD, nV, ent, cov, cavf,
                        (WALK && xw) ? kLjNoUser : decltype(ent)::kWild), t);
      ent = ent.skip(nD + 2u * nV);
    }
  } else {
    const uint32_t h0 = gptr(rec)[0];
    LjEnt32 e{rec + 1 + 2 * n_terms};
    for (uint32_t t = 0; t < n_terms; ++t) {
      const uint32_t nD = gptr(rec)[1 + 2 * t], nV = gptr(rec)[2 + 2 * t];
      fold(lj_term<CAV>(u, !(WALK && xw) && ((h0 >> (8 + t)) & 1u), nD, nV, e, cov, cavf,
                        (WALK && xw) ? kLjNoUser : LjEnt32::kWild), t);
      e = e.skip(nD + 2u * nV);
    }
  }
  return no ? (uint32_t)GCK_PERM_NO : cond ? (uint32_t)GCK_PERM_CONDITIONAL : (uint32_t)GCK_PERM_HAS;
}

// lj_decide for root M (its caveat plane and slot packing).
template <class Covers, class CavF>
__device__ __forceinline__ uint32_t lj_decide_root(const LjMeta& M, uint32_t u, uint32_t hdr, const uint32_t* rw,
                                                   const uint32_t* rec, const Covers& cov, const CavF& cavf) {
  if (M.pack)
    return M.cav ? lj_decide<true, true>(u, hdr, rw, rec, M.n_terms, M.neg, cov, cavf)
                 : lj_decide<false, true>(u, hdr, rw, rec, M.n_terms, M.neg, cov, cavf);
  return M.cav ? lj_decide<true, false>(u, hdr, rw, rec, M.n_terms, M.neg, cov, cavf)
               : lj_decide<false, false>(u, hdr, rw, rec, M.n_terms, M.neg, cov, cavf);
}

// The subject's direct grants on the resource's arrow-forest chain at the current revision, per
// term (2 bits each: 1 none, 2 a grant, 3 only grants through unresolved caveats), for a dirty
// subject whose overlay hit: its entries in the slot are stale, and this is what the flattening
// would list for it now. Every caveated grant met is evaluated (`cavf`), as lj_term evaluates
// every pair. kLjWalkDefer: a term without a program, an expiring grant (its visibility depends on
// the check's time), a chain past kLjChainDepth — the bundles decide the check.
constexpr uint32_t kLjWalkDefer = 0x80000000u;
#ifndef GCK_WALK_PRINTF
#define GCK_WALK_PRINTF 0
#endif
// EVAL: caveated grants are evaluated here (the kernels with the caveat plane, whose outcome tables
// are in LDS); without it a grant's caveat is taken from its stored-context outcome (a partial one
// is CONDITIONAL without check contexts, and defers the check with them: the global-memory
// evaluation, inlined into the walk, took the plain kernels from 75 to 101 VGPRs)
template <bool EVAL, class CavF>
__device__ __forceinline__ uint32_t lj_chain_walk(const LjChain* ch, uint32_t n_terms, const DevCSR* csrs,
                                                  uint32_t n_csrs, const unsigned long long* afp, uint32_t afp_n,
                                                  const uint8_t* cav_static, bool has_ctx, uint32_t r, uint32_t u,
                                                  const CavF& cavf) {
  uint32_t w = 0;
  for (uint32_t t = 0; t < n_terms; ++t) {  // (each term its own walk up the chain: a rare path)
    uint32_t l = ch->first[t];
    if (l >= kLjChainLvls) return kLjWalkDefer;
    uint32_t x = r, g = ch->lvl[l].af_base + r;
    bool hit = false, cond = false, done = false;
    for (uint32_t depth = 0; depth < kLjChainDepth && !done; ++depth) {
      if (GCK_WALK_PRINTF) printf("walk r=%u u=%u t=%u depth=%u g=%u/%u x=%u l=%u\n", r, u, t, depth, g, afp_n, x, l);
      if (g >= afp_n) return kLjWalkDefer;  // (never: the forest holds every object on a chain)
      // one depth in ~three rounds per four classes: the next hop, then the classes' row extents,
      // then the rows' first entries — each round's loads issued together (a loop of dependent
      // searches, class after class, took the config-5 join from 24 to 85-100 us)
      const unsigned long long pe = gptr(afp)[g];
      const LjChainLvl& L = ch->lvl[l];
      const uint32_t nc = min((uint32_t)L.n, kLjChainCls);
      constexpr uint32_t kB = 4, kRow = 2;  // classes per round of loads; entries read with the extent
      for (uint32_t c0 = 0; c0 < nc; c0 += kB) {
        const DevCSR* Rc[kB];
        uint32_t lo[kB], hi[kB], e2[kB][kRow];
#pragma unroll
        for (uint32_t b = 0; b < kB; ++b) {
          const uint32_t c = c0 + b;
          const uint32_t k = c < nc ? (uint32_t)L.csr[c] : 0u;
          if (k >= n_csrs) return kLjWalkDefer;  // (never: the classes are the snapshot's)
          Rc[b] = &csrs[k];
          lo[b] = hi[b] = 0u;
          if (c < nc && x < Rc[b]->n_rows) {
            lo[b] = csr_off(*Rc[b], x);
            hi[b] = csr_off(*Rc[b], x + 1);
          }
        }
#pragma unroll
        for (uint32_t b = 0; b < kB; ++b)
#pragma unroll
          for (uint32_t q = 0; q < kRow; ++q) e2[b][q] = lo[b] + q < hi[b] ? csr_nbr(*Rc[b], lo[b] + q) : kNone;
#pragma unroll
        for (uint32_t b = 0; b < kB; ++b) {
          if (lo[b] >= hi[b]) continue;
          uint32_t p = kNone;
#pragma unroll
          for (uint32_t q = 0; q < kRow; ++q)
            if (p == kNone && e2[b][q] == u) p = lo[b] + q;
          if (p == kNone && hi[b] - lo[b] > kRow) {  // (a longer row: searched)
            uint32_t probes = 0;
            p = row_find(*Rc[b], x, u, probes);
          }
          if (p == kNone) continue;
          if (!Rc[b]->is_ext) {
            hit = true;
            continue;
          }
          if (gptr(Rc[b]->exp_us)[p] != 0) return kLjWalkDefer;
          uint32_t sv;
          if (EVAL) {
            sv = cavf(csr_cav(*Rc[b], p));
          } else {  // (the instance's outcome under its stored context; a partial one without check
                    // contexts is CONDITIONAL, with them the bundles evaluate it)
            sv = cav_static ? (uint32_t)gptr(cav_static)[csr_cav(*Rc[b], p)] : 2u;
            if (sv == 2u && has_ctx) return kLjWalkDefer;
          }
          hit |= sv == 1u;
          cond |= sv == 2u;
        }
      }
      const uint32_t par = (uint32_t)pe, via = (uint32_t)(pe >> 32);
      const uint32_t nx = L.next;
      if (par == kNone || (uint32_t)L.arrow != via || nx >= kLjChainLvls) {
        done = true;
      } else {
        l = nx;
        x = par - ch->lvl[nx].af_base;
        g = par;
      }
    }
    if (!done) return kLjWalkDefer;  // (a chain past kLjChainDepth)
    w |= (hit ? 2u : cond ? 3u : 1u) << (2u * t);
  }
  return w;
}

// Per forest vertex one 64-B line (LjTables::anc): word 0 the number of its ancestors
// (kAncOver: more than kAncWords - 1, the line holds the first ones), words 1.. its parent, the
// parent's parent, ... as forest indices — the whole chain of a resource in one round.
constexpr uint32_t kAncWords = 16, kAncOver = 0x80000000u;
constexpr uint32_t kLjWalkLane = 0x40000000u;  // lj_chain_wave: the chain is longer than a line (per-lane walk)

// lj_chain_walk for the check of lane `o` by the whole wave (every lane calls it with the owner's
// values): the chain's objects come from the resource's ancestor line (one round), the tupleset
// of each hop from the parent edges (one round, a lane per depth), then a lane per (depth, class)
// pair reads the class's row extent and first entries (two rounds) — four rounds whatever the
// chain's length, where the lane's own walk takes two or three per depth (config 5: ~9 depths,
// the join 85-100 us with its walks against 24 us without). Same result encoding as
// lj_chain_walk; kLjWalkLane when the chain does not fit a line.
template <bool EVAL, class CavF>
__device__ __forceinline__ uint32_t lj_chain_wave(const LjChain* ch, uint32_t n_terms, const LjArgs& a, uint32_t r,
                                                  uint32_t u, int lane, const CavF& cavf_o, bool wild) {
  const uint32_t l0 = ch->first[0];
  if (l0 >= kLjChainLvls) return kLjWalkDefer;
  const uint32_t g0 = ch->lvl[l0].af_base + r;
  if (g0 >= a.afp_n) return kLjWalkDefer;
  const uint32_t word = lane < (int)kAncWords ? gptr(a.anc)[(size_t)g0 * kAncWords + (uint32_t)lane] : 0u;
  const uint32_t cw = (uint32_t)__shfl((int)word, 0, 64);
  if (cw & kAncOver) return kLjWalkLane;
  const uint32_t nd = cw + 1u;  // depths 0 .. cw
  // lane d < nd: the depth-d object and the tupleset of its parent edge
  const uint32_t gd = lane == 0 ? g0 : word;
  uint32_t via = kNone;
  if ((uint32_t)lane < nd && gd < a.afp_n) via = (uint32_t)(gptr(a.afp)[gd] >> 32);
  if ((uint32_t)lane < nd && gd >= a.afp_n) via = kNone - 1u;  // (never: flagged below)
  if (__ballot((uint32_t)lane < nd && gd >= a.afp_n) != 0ull) return kLjWalkDefer;
  uint32_t w = 0;
  for (uint32_t t = 0; t < n_terms; ++t) {
    // the term's level at each depth (uniform: the program is tiny and cached)
    uint32_t my_lvl = kLjChainEnd, l = ch->first[t];
    for (uint32_t d = 0; d < nd && l < kLjChainLvls; ++d) {
      if ((uint32_t)lane == d) my_lvl = l;
      const uint32_t v = (uint32_t)__shfl((int)via, (int)d, 64);
      const LjChainLvl& L = ch->lvl[l];
      l = ((uint32_t)L.arrow == v && d + 1u < nd) ? (uint32_t)L.next : (uint32_t)kLjChainEnd;
    }
    bool hit = false, cond = false, defer = false;
    // (depth, class) = (p / 8, p % 8), p < 128, for the subject; then, `wild`, for the wildcard —
    // unless the subject's own grants already decide the term
    for (uint32_t pass = 0; pass < (wild ? 4u : 2u); ++pass) {
      if (pass == 2u && __ballot(hit) != 0ull) break;
      const uint32_t pr = (uint32_t)lane + 64u * (pass & 1u), d = pr >> 3, c = pr & 7u;
      const uint32_t ld = (uint32_t)__shfl((int)my_lvl, (int)(d & 63u), 64);
      const uint32_t gdd = (uint32_t)__shfl((int)gd, (int)(d & 63u), 64);
      if (d >= nd || ld >= kLjChainLvls) continue;
      const LjChainLvl& L = ch->lvl[ld];
      if (c >= min((uint32_t)L.n, kLjChainCls)) continue;
      const uint32_t k = L.csr[c];
      if (k >= a.n_csrs) {
        defer = true;
        continue;
      }
      const DevCSR& R = a.csrs[k];
      const uint32_t x = gdd - L.af_base;
      if (x >= R.n_rows) continue;
      const uint32_t lo = csr_off(R, x), hi = csr_off(R, x + 1);
      if (lo >= hi) continue;
      uint32_t p;
      if (pass >= 2u) {  // the wildcard: the row's last entry (ids ascend, kWildcard is the largest)
        p = csr_nbr(R, hi - 1u) == kWildcard ? hi - 1u : kNone;
      } else {
        const uint32_t e0 = csr_nbr(R, lo), e1 = lo + 1u < hi ? csr_nbr(R, lo + 1u) : kNone;
        p = e0 == u ? lo : e1 == u ? lo + 1u : kNone;
        if (p == kNone && hi - lo > 2u) {  // (a longer row: searched)
          uint32_t probes = 0;
          p = row_find(R, x, u, probes);
        }
      }
      if (p == kNone) continue;
      if (!R.is_ext) {
        hit = true;
        continue;
      }
      if (gptr(R.exp_us)[p] != 0) {
        defer = true;
        continue;
      }
      uint32_t sv;
      if (EVAL) {
        sv = cavf_o(csr_cav(R, p));
      } else {
        sv = a.cav_static ? (uint32_t)gptr(a.cav_static)[csr_cav(R, p)] : 2u;
        if (sv == 2u && a.cx) defer = true;
      }
      hit |= sv == 1u;
      cond |= sv == 2u;
    }
    if (__ballot(defer) != 0ull) return kLjWalkDefer;
    const bool th = __ballot(hit) != 0ull, tc = __ballot(cond) != 0ull;
    w |= (th ? 2u : tc ? 3u : 1u) << (2u * t);
  }
  return w;
}

// A dirty subject's check whose overlay hit, decided again: the slot without the subject's own
// entries, joined per term with the chain walk. 0: deferred to the bundles.
template <bool EVAL, class Covers, class CavF>
__device__ __forceinline__ uint32_t lj_redecide(const LjMeta& M, const LjArgs& a, uint32_t r, uint32_t u, uint32_t hdr,
                                                const uint32_t* rw, const uint32_t* rec, const Covers& cov,
                                                const CavF& cavf, uint32_t w, bool wild) {
  // (w: the wave's walk, lj_chain_wave; kLjWalkLane: the lane walks the chain itself. wild: the
  // slot's wildcard entries are stale, kLjHdrWildDirty — the walk reads the wildcard's grants too)
  if (w & kLjWalkLane) {
    if (wild) return 0u;  // (the lane's walk for the subject only: a wildcard walk there took the plain
                          // kernels from 80 to 84 VGPRs, 6 waves per SIMD to 5 — a chain this long defers)
    w = lj_chain_walk<EVAL>(M.chain, M.n_terms, a.csrs, a.n_csrs, a.afp, a.afp_n, a.cav_static, a.cx != nullptr, r,
                            u, cavf);
  }
  if (w & kLjWalkDefer) return 0u;
  if (M.pack)
    return M.cav ? lj_decide<true, true, true>(kLjNoUser, hdr, rw, rec, M.n_terms, M.neg, cov, cavf, w, wild)
                 : lj_decide<false, true, true>(kLjNoUser, hdr, rw, rec, M.n_terms, M.neg, cov, cavf, w, wild);
  return M.cav ? lj_decide<true, false, true>(kLjNoUser, hdr, rw, rec, M.n_terms, M.neg, cov, cavf, w, wild)
               : lj_decide<false, false, true>(kLjNoUser, hdr, rw, rec, M.n_terms, M.neg, cov, cavf, w, wild);
}

// lj_decide for one check by the whole wave (no caveat plane: M.cav == 0), when its walk is long
// for one lane — an extension record in HBM or a cover list (the slowest waves of configs 2 and 3:
// one lane scanned hundreds of entries while 63 waited, tools/analyze_lj.py). The check's user
// and resource slot words are in LDS (`slots`: kUSlotWords, then the resource's); per term the
// lanes share the users (u among them), and the intervals against the covers — lanes over the
// intervals when the covers are inline (every lane unpacks them), over the list's entries when
// they are a list. Same tri-state algebra as lj_decide without caveats: HAS or NO.
template <int BITS>
__device__ __noinline__ uint32_t lj_decide_wave(const LjMeta& M, uint32_t u, const uint32_t* slots, int lane) {
  const uint32_t* uw = slots;
  const uint32_t* rw = slots + kUSlotWords;
  const uint32_t hdr = rw[0];
  const bool ext = (hdr & kLjHdrExt) != 0u;
  const uint32_t* rec = ext ? M.rext + rw[1] : nullptr;
  const bool list = (uw[0] & kSlotList) != 0u;
  const uint32_t* lp = list ? M.ulist + slot_list_off(uw) : nullptr;
  const uint32_t ng = list ? slot_list_count(uw[0]) : uw[0];
  uint32_t cov[kSlotGMax];
  if (!list) {
    uint32_t w[kUSlotWords];
#pragma unroll
    for (uint32_t q = 0; q < kUSlotWords; ++q) w[q] = uw[q];
    slot_unpack<BITS>(w, cov);
  }
  const uint32_t n_terms = M.n_terms;
  const uint32_t h0 = ext ? gptr(rec)[0] : 0u;
  uint32_t off = 0;  // the term's first entry
  bool no = false;
  for (uint32_t t = 0; t < n_terms; ++t) {
    uint32_t nD, nV;
    bool hit;
    if (ext) {
      nD = gptr(rec)[1 + 2 * t];
      nV = gptr(rec)[2 + 2 * t];
      hit = (h0 >> (8 + t)) & 1u;
    } else {
      const uint32_t f = hdr >> (10u * t);
      nD = f & 31u;
      nV = (f >> 5) & 15u;
      hit = (f >> 9) & 1u;
    }
    // entry k of the term
    auto ent = [&](uint32_t k) -> uint32_t {
      if (ext) return gptr(rec)[1 + 2 * n_terms + off + k];
      if (M.pack) return LjEnt24{rw, off}[k];
      return rw[1 + off + k];
    };
    for (uint32_t k = (uint32_t)lane; k < nD && !hit; k += 64u) hit = ent(k) == u;
    if (list) {
      for (uint32_t k = (uint32_t)lane; k < ng && !hit; k += 64u) {
        const uint32_t c = gptr(lp)[k];
        for (uint32_t j = 0; j < nV && !hit; ++j) hit = c - ent(nD + 2 * j) < ent(nD + 2 * j + 1);
      }
    } else {
      for (uint32_t j = (uint32_t)lane; j < nV && !hit; j += 64u) {
        const uint32_t lo = ent(nD + 2 * j), len = ent(nD + 2 * j + 1);
#pragma unroll
        for (int k = 0; k < slot_cap<BITS>(); ++k) hit |= (uint32_t)k < ng && cov[k] - lo < len;
      }
    }
    hit = __ballot(hit) != 0ull;
    const bool neg = (M.neg >> t) & 1u;
    no |= hit == neg;  // (a term not reached, or a subtracted term reached)
    off += nD + 2u * nV;
  }
  return no ? (uint32_t)GCK_PERM_NO : (uint32_t)GCK_PERM_HAS;
}

// lj_decide_wave for a caveated root, in the kernels with the caveat plane only (inlined there: in
// the kernels without it, it had raised the register count from 73 to 106). The check's user and resource slot words are in
// LDS (`slots`: kUSlotWords, then the resource's); per term the lanes share the users (u among
// them; a caveated pair — a word with Ent::kCav, then its instance — evaluated by the lane holding
// its first word through `cavf`), and the intervals against the covers — lanes over the intervals
// when the covers are inline (every lane unpacks them), over the list's entries when they are a
// list. The tri-state algebra of lj_decide: HAS, NO or CONDITIONAL.
template <int BITS, class CavF>
__device__ __forceinline__ uint32_t lj_decide_wave_cav(const LjMeta& M, uint32_t u, const uint32_t* slots, int lane,
                                                       const CavF& cavf) {
  const uint32_t* uw = slots;
  const uint32_t* rw = slots + kUSlotWords;
  const uint32_t hdr = rw[0];
  const bool ext = (hdr & kLjHdrExt) != 0u;
  const uint32_t* rec = ext ? M.rext + rw[1] : nullptr;
  const bool list = (uw[0] & kSlotList) != 0u;
  const uint32_t* lp = list ? M.ulist + slot_list_off(uw) : nullptr;
  const uint32_t ng = list ? slot_list_count(uw[0]) : uw[0];
  uint32_t cov[kSlotGMax];
  if (!list) {
    uint32_t w[kUSlotWords];
#pragma unroll
    for (uint32_t q = 0; q < kUSlotWords; ++q) w[q] = uw[q];
    slot_unpack<BITS>(w, cov);
  }
  const uint32_t n_terms = M.n_terms;
  const uint32_t h0 = ext ? gptr(rec)[0] : 0u;
  // the entries' caveated-pair marks: 24-bit fields (LjEnt24) or words (LjEnt32)
  const bool p24 = !ext && M.pack;
  const uint32_t kcav = p24 ? LjEnt24::kCav : LjEnt32::kCav, kwild = p24 ? LjEnt24::kWild : LjEnt32::kWild;
  uint32_t off = 0;  // the term's first entry
  bool no = false, cond_any = false;
  for (uint32_t t = 0; t < n_terms; ++t) {
    uint32_t nD, nV;
    bool hit, cond = false;
    if (ext) {
      nD = gptr(rec)[1 + 2 * t];
      nV = gptr(rec)[2 + 2 * t];
      hit = (h0 >> (8 + t)) & 1u;
    } else {
      const uint32_t f = hdr >> (10u * t);
      nD = f & 31u;
      nV = (f >> 5) & 15u;
      hit = (f >> 9) & 1u;
    }
    // entry k of the term
    auto ent = [&](uint32_t k) -> uint32_t {
      if (ext) return gptr(rec)[1 + 2 * n_terms + off + k];
      if (p24) return LjEnt24{rw, off}[k];
      return rw[1 + off + k];
    };
    if (M.cav) {
      // every caveated pair of the subject is evaluated (as lj_term: SpiceDB evaluates each
      // caveated relationship it meets); a word after a pair's first is its instance
      for (uint32_t k = (uint32_t)lane; k < nD; k += 64u) {
        const uint32_t w = ent(k);
        if (w & kcav) {
          const uint32_t x = w & ~kcav;
          if (x == u || x == kwild) {
            const uint32_t sv = cavf(ent(k + 1));
            hit |= sv == 1u;
            cond |= sv == 2u;
          }
        } else if (!(k && (ent(k - 1) & kcav))) {
          hit |= w == u;
        }
      }
    } else {
      for (uint32_t k = (uint32_t)lane; k < nD && !hit; k += 64u) hit = ent(k) == u;
    }
    if (list) {
      for (uint32_t k = (uint32_t)lane; k < ng && !hit; k += 64u) {
        const uint32_t c = gptr(lp)[k];
        for (uint32_t j = 0; j < nV && !hit; ++j) hit = c - ent(nD + 2 * j) < ent(nD + 2 * j + 1);
      }
    } else {
      for (uint32_t j = (uint32_t)lane; j < nV && !hit; j += 64u) {
        const uint32_t lo = ent(nD + 2 * j), len = ent(nD + 2 * j + 1);
#pragma unroll
        for (int k = 0; k < slot_cap<BITS>(); ++k) hit |= (uint32_t)k < ng && cov[k] - lo < len;
      }
    }
    hit = __ballot(hit) != 0ull;
    cond = __ballot(cond) != 0ull;
    uint32_t v = hit ? 2u : cond ? 3u : 1u;
    if ((M.neg >> t) & 1u) v = v == 2u ? 1u : v == 1u ? 2u : v;
    no |= v == 1u;
    cond_any |= v == 3u;
    off += nD + 2u * nV;
  }
  return no ? (uint32_t)GCK_PERM_NO : cond_any ? (uint32_t)GCK_PERM_CONDITIONAL : (uint32_t)GCK_PERM_HAS;
}

// One wavefront per CPW checks (32; 16 is kept compilable for measurements), 4 per block. SW: resource slot words (16 or 32), the
// same for every root of the snapshot. Per check 1 + SW / 16 lines: its user slot and its resource
// slot, fetched by four lanes each (one 16-B chunk per lane, every line one request), staged in LDS.
template <int BITS, uint32_t SW, uint32_t CPW, bool CL = false>
__global__ void __launch_bounds__(kBlock) k_label_join(LjArgs a) {
  static_assert(CPW == 16 || CPW == 32, "checks per wave");
  const unsigned long long t_start = (GCK_BUNDLE_TIMING && a.timing) ? wall_clock64() : 0ull;
  __shared__ std::conditional_t<CL, LjCavLds, LjNoCavLds> s_cav;
  constexpr uint32_t kLines = 1u + SW / 16u;
  constexpr uint32_t kWords = kUSlotWords + SW;
  // a check's words in LDS are kStride apart: +4 words spread the lanes' reads of their own slots
  // over the banks (ds_read_b32 banks are word mod 32: a stride of 48 words put 32 lanes on 2 banks,
  // of 32 words on one; 52 puts them on 8) and keep the 16-B alignment of the staging stores
  constexpr uint32_t kStride = kWords + 4u;
  constexpr uint32_t kR = CPW * kLines / 16u;  // load instructions per lane (16 lines each)
  __shared__ __attribute__((aligned(16))) unsigned char s_tab[kLjLdsBytes];
  __shared__ __attribute__((aligned(16))) uint32_t s_stage[kWaves][CPW * kStride];
  __shared__ unsigned long long s_ua[kWaves][CPW], s_ra[kWaves][CPW];
  __shared__ unsigned s_pub[2];  // (kPubBySignal) the block's deferred checks, a bad context slot
  if (threadIdx.x < 2) s_pub[threadIdx.x] = 0u;
  // the wave's items are requested before the table: both loads in flight together
  const uint32_t w0 = (blockIdx.x * kWaves + (threadIdx.x >> 6)) * CPW;
  const bool list = a.list != 0u;  // a list batch (closure.inc cj_block): its range form has no `pairs`
  const bool uni = a.pairs != nullptr || list;  // a uniform batch (a scalar branch)
  const uint32_t item_bytes = w0 < a.n ? min(CPW, a.n - w0) * 20u : 0u;
  const unsigned char* ibase = reinterpret_cast<const unsigned char*>(a.items) + (size_t)w0 * 20u;
  const bool items_fast = !uni && ((uintptr_t)a.items & 15u) == 0 && item_bytes == CPW * 20u;
  u32x4 item_chunk{0u, 0u, 0u, 0u};
  if (items_fast && (threadIdx.x & 63u) < CPW * 20u / 16u)
    item_chunk = *(const GCK_GLOBAL u32x4*)(ibase + (threadIdx.x & 63u) * 16u);
  // (not a cross batch's lanes: `pairs` is then the id block; nor a list batch's: the id list, or null)
  const bool grid = uni && a.n_shapes == 0u && a.cols != 0u && !list;
  if (uni && (threadIdx.x & 63u) < CPW && w0 + (threadIdx.x & 63u) < a.n && !grid && !list) {  // (a uniform batch: the lane's pair)
    const unsigned long long pr = *(const GCK_GLOBAL unsigned long long*)(a.pairs + 2ull * (w0 + (threadIdx.x & 63u)));
    item_chunk.x = (uint32_t)pr;
    item_chunk.y = (uint32_t)(pr >> 32);
  }
  // a cross batch (closure.inc cj_block): the lane's resource id and its row's subject id from the
  // id block instead, in the same round (in the chunk's spare registers until the table's barrier,
  // as there); a lane whose column is padding stays idle
  bool grid_on = true;
  if (__builtin_expect(grid, 0)) {
    uint32_t row, col;
    cross_rc((uint32_t)__builtin_amdgcn_readfirstlane((int)(w0 >> 5)), (w0 + threadIdx.x) & 31u, (a.cols + 31u) >> 5, row, col);
    grid_on = col < a.cols;
    if ((threadIdx.x & 63u) < CPW && w0 + (threadIdx.x & 63u) < a.n && grid_on) {
      item_chunk.z = *(const GCK_GLOBAL uint32_t*)(a.pairs + col);
      item_chunk.w = *(const GCK_GLOBAL uint32_t*)(a.pairs + cross_sub_off(a.cols) + row);
    }
  }
  // a list batch (closure.inc cj_block): the lane's one id — in range form computed — and the fixed
  // id, in the chunk's spare registers until the table's barrier
  if (__builtin_expect(list, 0)) {
    if ((threadIdx.x & 63u) < CPW && w0 + (threadIdx.x & 63u) < a.n) {
      item_chunk.w = a.u_fixed;
      if (a.list & kListRange) item_chunk.z = a.cols + w0 + (threadIdx.x & 63u);
      else item_chunk.z = *(const GCK_GLOBAL uint32_t*)(a.pairs + w0 + (threadIdx.x & 63u));
    }
  }
  // a shaped batch (closure.inc cj_block): the lane's index byte, and entry l of the shape table by
  // lane l < n_shapes, in the same round; the entries are staged in the wave's own stage region
  // (idle in this mode until the slots) and read by index after the table's barrier
  const bool shaped = uni && a.n_shapes != 0u;  // (a list batch's n_shapes is 0)
  const uint32_t n_shapes = min(a.n_shapes, (uint32_t)GCK_MAX_SHAPES);
  static_assert(CPW * kStride >= GCK_MAX_SHAPES * 4u, "the stage region holds the shape table");
  u32x4 shape_ent{0u, 0u, 0u, 0u};
  if (__builtin_expect(shaped, 0)) {
    if ((threadIdx.x & 63u) < CPW && w0 + (threadIdx.x & 63u) < a.n)
      item_chunk.z = *(const GCK_GLOBAL uint8_t*)(a.shape_of + w0 + (threadIdx.x & 63u));
    if ((threadIdx.x & 63u) < n_shapes) shape_ent = *(const GCK_GLOBAL u32x4*)(a.shapes + (threadIdx.x & 63u));
  }
  for (uint32_t k = threadIdx.x; k < a.table_bytes / 4; k += kBlock)
    reinterpret_cast<uint32_t*>(s_tab)[k] = gptr(reinterpret_cast<const uint32_t*>(a.table))[k];
  if (__builtin_expect(shaped, 0) && (threadIdx.x & 63u) < n_shapes)
    *reinterpret_cast<u32x4*>(&s_stage[threadIdx.x >> 6][(threadIdx.x & 63u) * 4u]) = shape_ent;
  uint32_t cl_nctx = 0, cl_ndist = 0;
  if constexpr (CL) {  // (the launcher checked the sizes against kLjCav*)
    const Ctx& c = *a.cx;
    cl_nctx = c.n_ctx;
    cl_ndist = c.n_dist;
    for (uint32_t k = threadIdx.x; k < a.cav_n; k += kBlock) {
      s_cav.st[k] = gptr(c.cav_static)[k];
      const uint32_t r = gptr(c.cav_row)[k];
      s_cav.row[k] = (uint16_t)min(r, 0xFFFFu);
    }
    for (uint32_t k = threadIdx.x; k < a.cav_rows * cl_ndist; k += kBlock) s_cav.dyn[k] = gptr(c.cav_dyn)[k];
    for (uint32_t k = threadIdx.x; k < cl_nctx; k += kBlock) s_cav.slot[k] = (uint8_t)gptr(c.cav_slot)[k];
  }
  __syncthreads();
  if (__builtin_expect(grid, 0)) item_chunk.x = item_chunk.z, item_chunk.y = item_chunk.w;
  if (__builtin_expect(list, 0)) {  // (resource id, subject id): the varying id and the fixed one
    const bool sub = (a.list & kListSubject) != 0u;
    item_chunk.x = sub ? item_chunk.w : item_chunk.z;
    item_chunk.y = sub ? item_chunk.z : item_chunk.w;
  }
  const unsigned long long t_tab = (GCK_BUNDLE_TIMING && a.timing) ? wall_clock64() : 0ull;
  const uint16_t* root = reinterpret_cast<const uint16_t*>(s_tab);
  const LjMeta* meta = reinterpret_cast<const LjMeta*>(s_tab + a.o_meta);
  const int wib = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t* const stage = s_stage[wib];
  const uint32_t i = w0 + (uint32_t)lane;
  const bool active = (uint32_t)lane < CPW && i < a.n && grid_on;
  // ---- the wave's items: one contiguous block of CPW x 20 B -------------------------------------
  if (uni) {
    // (the pairs are in registers)
  } else if (items_fast) {
    if ((uint32_t)lane < CPW * 20u / 16u) *reinterpret_cast<u32x4*>(&stage[lane * 4u]) = item_chunk;
  } else if (active) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.items + i);
    for (uint32_t q = 0; q < 5u; ++q) stage[lane * 5u + q] = gptr(src)[q];
  }
  lds_wave_fence();
  gck_item it{};
  if (active && uni) {
    if (__builtin_expect(shaped, 0)) {
      const uint32_t sb = min(item_chunk.z, n_shapes - 1u);  // clamped before the lookup
      it = shaped_item(*reinterpret_cast<const u32x4*>(&stage[sb * 4u]), item_chunk.z >= n_shapes, item_chunk.x, item_chunk.y);
    } else {
      it = uniform_item(a.u_rp, a.u_ss, a.u_ctx, item_chunk.x, item_chunk.y);
    }
    if (a.cx) gptr_w(a.cx->cav_flag)[i] = 0;
  } else if (active) {
    uint32_t iw[5];
    for (uint32_t q = 0; q < 5u; ++q) iw[q] = stage[lane * 5u + q];
    __builtin_memcpy(&it, iw, sizeof(it));
    // a batch with check contexts: the check's caveat flag starts cleared here (set below, or by
    // the bundles after this kernel, when an evaluation fails) — no memset on a stream before
    if (a.cx) gptr_w(a.cx->cav_flag)[i] = 0;
  }
  if (a.bad_slot && check_slots(a.bad_slot, a.slot_limit, active, it, w0, lane) && lane == 0) atomicOr(&s_pub[1], 1u);
  bool ctr_touched = false;  // a device counter this lane's check wrote (the caveat plane's)
  // ---- addresses: a label root, the subject type of its slots, ids within them ------------------
  unsigned long long ua = 0, ra = 0;
  uint32_t hub_w = 0;  // hub root: word of the vertex's label within the fetched line
  uint32_t dword = 0;  // the subject's word of the dirty set: loaded now, tested once the slots are in
  LjMeta M{};
  uint32_t droot = 0;  // (the root's index in the table: a heavy check's, for the wave below)
  if (active && it.permission < a.n_fwd && it.subject_relation == kEllipsis) {
    const uint32_t d = root[it.permission];
    if (d != 0xFFFFu) {
      droot = d;
      M = meta[d];
      if (it.resource_type == M.rtype && it.subject_type == M.utype && it.subject_id < M.u_rows &&
          it.resource_id < M.r_rows) {
        if (M.n_terms && a.dirty) dword = gptr(a.dirty)[it.subject_id >> 5];
        ua = (unsigned long long)(uintptr_t)(M.uslot + (size_t)it.subject_id * kUSlotWords);
        if (M.n_terms) {
          ra = (unsigned long long)(uintptr_t)(M.rslot + (size_t)it.resource_id * SW);
        } else {  // hub root: the line holding the vertex's (pre, end) label
          const unsigned long long la = (unsigned long long)(uintptr_t)(M.rslot + 2 * (size_t)it.resource_id);
          ra = la & ~63ull;
          hub_w = (uint32_t)(la & 63ull) / 4u;
        }
      }
    }
  }
  if ((uint32_t)lane < CPW) {
    s_ua[wib][lane] = ua;
    s_ra[wib][lane] = ra;
  }
  lds_wave_fence();  // (the items are in registers: the stage region takes the slots)
  uint32_t res = 0;  // GCK_PERM_HAS / NO / CONDITIONAL, 0 deferred
  bool dirty = false;
  unsigned long long t_slots = 0;
  bool used_list = false, used_ext = false;  // (TIMING builds: what the wave's checks read)
  bool heavy = false;  // decided by the whole wave below (an extension record or a cover list)
  bool why_over = false, why_dirty = false, why_hit = false;  // (TIMING builds: why a check was deferred)
  // a caveated pair of the subject: its caveat under the check's context (engine.hip cav_state;
  // from the LDS copies of the tables when they fit)
  const auto cavf = [&](uint32_t cav) -> uint32_t {
    if constexpr (CL) {
      const uint32_t s = s_cav.st[cav];
      if (s != 2u || cl_nctx == 0) return s;
      const uint32_t slot = it.context_slot;
      if (slot == 0 || slot > cl_nctx) return 2u;
      const uint32_t v = s_cav.dyn[(uint32_t)s_cav.row[cav] * cl_ndist + s_cav.slot[slot - 1]];
      if (v == 3u) {
        gptr_w(a.cx->cav_flag)[i] = 1;
        atomicAdd(&a.cx->ctr->cav_errors, 1u);
        ctr_touched = true;
      }
      return v > 2u ? 2u : v;
    } else {
      if (!a.cx) return 2u;
      const uint32_t v = cav_state(*a.cx, cav, i);
      // (an unresolved dynamic caveat may have counted a lazy request or an evaluation error)
      ctr_touched |= v == 2u && a.cx->n_ctx != 0u;
      return v;
    }
  };
  if (__ballot(ua != 0) != 0) {
    u32x4 y[kR];
#pragma unroll
    for (uint32_t r = 0; r < kR; ++r) {  // line k = 16 r + lane / 4: check k / kLines, part k % kLines
      const uint32_t k = 16u * r + ((uint32_t)lane >> 2), chk = k / kLines, part = k - chk * kLines;
      const unsigned long long b = part == 0u ? s_ua[wib][chk] : s_ra[wib][chk];
      y[r] = b ? slot_load((const GCK_GLOBAL u32x4*)(b + (part ? (part - 1u) * 64u : 0u) + ((uint32_t)lane & 3u) * 16u))
               : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (uint32_t r = 0; r < kR; ++r) {
      const uint32_t k = 16u * r + ((uint32_t)lane >> 2), chk = k / kLines, part = k - chk * kLines;
      *reinterpret_cast<u32x4*>(&stage[chk * kStride + part * 16u + ((uint32_t)lane & 3u) * 4u]) = y[r];
    }
    lds_wave_fence();
    if (GCK_BUNDLE_TIMING && a.timing) t_slots = wall_clock64();
    if (ua) {
      const uint32_t* uw_s = &stage[(uint32_t)lane * kStride];
      const uint32_t* rw = uw_s + kUSlotWords;
      uint32_t uw[kUSlotWords];
#pragma unroll
      for (uint32_t q = 0; q < kUSlotWords; q += 4) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(&uw_s[q]);
        uw[q] = v.x, uw[q + 1] = v.y, uw[q + 2] = v.z, uw[q + 3] = v.w;
      }
      const uint32_t hdr = M.n_terms ? rw[0] : (rw[hub_w + 1] & kLjDeep);  // (a deep hub vertex: deferred)
      // the subject's grants changed since the tables were built: decided here all the same when
      // the arrow forest can tell whether a changed object lies on the resource's flattening
      // (round 2 below), else the bundles
      dirty = (dword >> (it.subject_id & 31u)) & 1u;
      if (GCK_BUNDLE_TIMING) {
        why_over = ((hdr | uw[0]) & kSlotOverflow) != 0u;
        why_dirty = !why_over && dirty && !(M.apre && a.dov);
      }
      if (!((hdr | uw[0]) & kSlotOverflow) && (!dirty || (M.apre && a.dov))) {
        const uint32_t* rec = (hdr & kLjHdrExt) ? M.rext + rw[1] : nullptr;
        if (GCK_BUNDLE_TIMING) {
          used_list = (uw[0] & kSlotList) != 0u;
          used_ext = rec != nullptr;
        }
        if (!M.n_terms) {  // hub root: a cover of the subject in the vertex's own interval
          const uint32_t lo = rw[hub_w] & ~kSlotOverflow, len = rw[hub_w + 1] - lo;
          bool has;
          if (uw[0] & kSlotList) {
            has = LjListCovers{M.ulist + slot_list_off(uw), slot_list_count(uw[0])}.any_in(lo, len);
          } else {
            LjInlineCovers<BITS> ci;
            slot_unpack<BITS>(uw, ci.p);
            ci.ng = uw[0];
            has = ci.any_in(lo, len);
          }
          res = has ? 2u : 1u;
        } else if ((!M.cav || CL) && (rec || ((uw[0] & kSlotList) && !(M.cav && M.pack)))) {
          // (a long walk for one lane: the wave shares it, lj_decide_wave — a caveated root's only
          // in the kernels with the caveat plane (lj_decide_wave_cav, inlined: in the others it
          // took the kernel from 73 to 106 VGPRs, 6 waves per SIMD down to 4, and config 2 from
          // 11.9 to 10.4 G checks/s; `profiles/r05/lj_noinline/`), and not for the 24-bit inline
          // fields of a caveated root, where an instance field may carry the pair mark and only the
          // entry-by-entry walk tells the pairs apart)
          heavy = true;
        } else if (uw[0] & kSlotList) {
          LjListCovers cl{M.ulist + slot_list_off(uw), slot_list_count(uw[0])};
          res = lj_decide_root(M, it.subject_id, hdr, rw, rec, cl, cavf);
        } else {
          LjInlineCovers<BITS> ci;
          slot_unpack<BITS>(uw, ci.p);
          ci.ng = uw[0];
          res = lj_decide_root(M, it.subject_id, hdr, rw, rec, ci, cavf);
        }
      }
    }
    // the heavy checks, one at a time, each by the whole wave (its slots are in the stage region)
    for (unsigned long long hm = __ballot(heavy); hm; hm &= hm - 1ull) {
      const int o = __ffsll((long long)hm) - 1;
      const LjMeta& Mo = meta[__shfl((int)droot, o, 64)];
      const uint32_t u_o = (uint32_t)__shfl((int)it.subject_id, o, 64);
      uint32_t r;
      if constexpr (CL) {
        if (Mo.cav) {
          const uint32_t io = (uint32_t)__shfl((int)i, o, 64), slot_o = (uint32_t)__shfl((int)it.context_slot, o, 64);
          // the owner's caveat outcomes (the per-lane `cavf` above, for the owner's check)
          const auto cavf_o = [&](uint32_t cav) -> uint32_t {
            const uint32_t st = s_cav.st[cav];
            if (st != 2u || cl_nctx == 0) return st;
            if (slot_o == 0 || slot_o > cl_nctx) return 2u;
            const uint32_t v = s_cav.dyn[(uint32_t)s_cav.row[cav] * cl_ndist + s_cav.slot[slot_o - 1]];
            if (v == 3u) {
              gptr_w(a.cx->cav_flag)[io] = 1;
              atomicAdd(&a.cx->ctr->cav_errors, 1u);
              ctr_touched = true;
            }
            return v > 2u ? 2u : v;
          };
          r = lj_decide_wave_cav<BITS>(Mo, u_o, &stage[(uint32_t)o * kStride], lane, cavf_o);
        } else {
          r = lj_decide_wave<BITS>(Mo, u_o, &stage[(uint32_t)o * kStride], lane);
        }
      } else {
        r = lj_decide_wave<BITS>(Mo, u_o, &stage[(uint32_t)o * kStride], lane);
      }
      if (lane == o) res = r;
    }
  }
  // ---- round 2, dirty subjects only: the objects whose grants of the subject changed since the
  // tables were built (their arrow-forest intervals) against the resource's position. The slots'
  // answer stands unless one of them is the resource or an object its flattening visited (an
  // ancestor in the forest), or the subject's list overflowed.
  const bool dchk = dirty && res != 0u;
  // the resource's own wildcard grants changed (kLjHdrWildDirty): a slot answer to take again with
  // the wildcard's current grants (round 3). (Its header from the stage, the root from LDS: nothing
  // of it stays live through round 1, whose registers bound the kernel's occupancy.)
  bool wdirty = false;
  if (res != 0u) {
    const LjMeta& Mw = meta[droot];
    const uint32_t h = stage[(uint32_t)lane * kStride + kUSlotWords];
    wdirty = Mw.n_terms && (h & kLjHdrWildDirty) && ((h & kLjHdrExt) || Mw.n_terms < 3u) && Mw.chain != nullptr;
  }
  bool walk = false;  // an overlay hit decided again from the current rows (round 3)
  if (__ballot(dchk) != 0 && dchk) {
    const GCK_GLOBAL u32x4* L = (const GCK_GLOBAL u32x4*)(a.dov + (size_t)it.subject_id * kDovWords);
    const u32x4 q0 = L[0], q1 = L[1], q2 = L[2], q3 = L[3];
    const uint32_t pre = gptr(M.apre)[2 * (size_t)it.resource_id];
    const uint32_t w[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
    const uint32_t nc = min(w[0] & ~kDovOver, kDovPairs);
    bool hit = (w[0] & kDovOver) != 0u;
#pragma unroll
    for (uint32_t k = 0; k < 7u; ++k) hit |= k < nc && pre - w[2 + 2 * k] < w[3 + 2 * k] - w[2 + 2 * k];
    if (!hit && nc > 7u) {  // (the second line: a third round, for subjects with more than 7)
      const u32x4 q4 = L[4], q5 = L[5], q6 = L[6], q7 = L[7];
      const uint32_t v[16] = {q4.x, q4.y, q4.z, q4.w, q5.x, q5.y, q5.z, q5.w, q6.x, q6.y, q6.z, q6.w, q7.x, q7.y, q7.z, q7.w};
#pragma unroll
      for (uint32_t k = 0; k < 8u; ++k) hit |= 7u + k < nc && pre - v[2 * k] < v[2 * k + 1] - v[2 * k];
    }
    // a hit (or an overflowed list): the subject's entries in the slot may be stale — with a chain
    // program the check is decided again below from the current rows, else by the bundles
    if (hit) res = 0u;
    walk = hit && meta[droot].chain != nullptr;
    if (GCK_BUNDLE_TIMING) why_hit = hit && !walk;
  }
  walk |= wdirty;
  // ---- round 3, overlay hits: the subject's direct grants on the resource's chain, read from the
  // current revision's rows (lj_chain_walk), joined with the rest of the slot (its stage copy)
  uint32_t wres = kLjWalkLane;  // (a lane's walk result: by the whole wave when the ancestors fit a line)
  if (a.anc) {
    for (unsigned long long wm = __ballot(walk); wm; wm &= wm - 1ull) {
      const int o = __ffsll((long long)wm) - 1;
      const LjMeta& Mo = meta[__shfl((int)droot, o, 64)];
      const uint32_t r_o = (uint32_t)__shfl((int)it.resource_id, o, 64), u_o = (uint32_t)__shfl((int)it.subject_id, o, 64);
      const bool wild_o = __shfl((int)wdirty, o, 64) != 0;
      uint32_t x;
      if constexpr (CL) {
        const uint32_t io = (uint32_t)__shfl((int)i, o, 64), slot_o = (uint32_t)__shfl((int)it.context_slot, o, 64);
        const auto cavf_o = [&](uint32_t cav) -> uint32_t {  // (the owner's check: cavf for its context)
          const uint32_t st = s_cav.st[cav];
          if (st != 2u || cl_nctx == 0) return st;
          if (slot_o == 0 || slot_o > cl_nctx) return 2u;
          const uint32_t v = s_cav.dyn[(uint32_t)s_cav.row[cav] * cl_ndist + s_cav.slot[slot_o - 1]];
          if (v == 3u) {
            gptr_w(a.cx->cav_flag)[io] = 1;
            atomicAdd(&a.cx->ctr->cav_errors, 1u);
            ctr_touched = true;
          }
          return v > 2u ? 2u : v;
        };
        x = lj_chain_wave<true>(Mo.chain, Mo.n_terms, a, r_o, u_o, lane, cavf_o, wild_o);
      } else {
        x = lj_chain_wave<false>(Mo.chain, Mo.n_terms, a, r_o, u_o, lane, cavf, wild_o);
      }
      if (lane == o) wres = x;
    }
  }
  if (__ballot(walk) != 0 && walk) {
    const LjMeta& M3 = meta[droot];  // (from LDS again: nothing of the root stays live for this rare round)
    const uint32_t* uw_s = &stage[(uint32_t)lane * kStride];
    const uint32_t* rw = uw_s + kUSlotWords;
    uint32_t uw[kUSlotWords];
#pragma unroll
    for (uint32_t q = 0; q < kUSlotWords; q += 4) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(&uw_s[q]);
      uw[q] = v.x, uw[q + 1] = v.y, uw[q + 2] = v.z, uw[q + 3] = v.w;
    }
    const uint32_t hdr = rw[0];
    const uint32_t* rec = (hdr & kLjHdrExt) ? M3.rext + rw[1] : nullptr;
    if (uw[0] & kSlotList) {
      LjListCovers cl{M3.ulist + slot_list_off(uw), slot_list_count(uw[0])};
      res = lj_redecide<CL>(M3, a, it.resource_id, it.subject_id, hdr, rw, rec, cl, cavf, wres, wdirty);
    } else {
      LjInlineCovers<BITS> ci;
      slot_unpack<BITS>(uw, ci.p);
      ci.ng = uw[0];
      res = lj_redecide<CL>(M3, a, it.resource_id, it.subject_id, hdr, rw, rec, ci, cavf, wres, wdirty);
    }
    if (GCK_BUNDLE_TIMING) why_hit = res == 0u;
  }
  const unsigned long long t_dec = (GCK_BUNDLE_TIMING && a.timing) ? wall_clock64() : 0ull;
  if (uni) {
    packed_store(a.out_packed, w0, active ? res : 0u, lane, CPW, a.n);
  } else if (active && res) {
    store_result(a.out_perm + i, (uint8_t)res, (a.coherent & kPubCoherent) != 0u);
    store_result(a.out_err + i, (int32_t)GCK_ITEM_OK, (a.coherent & kPubCoherent) != 0u);
  }
  const uint32_t at = wave_append(a.n_deferred, active && !res);  // (one counter add per wave)
  if (active && !res) a.deferred[at] = i;
  if (active && !res && uni) {  // the check's item where the bundle stages read it (its pair read again)
    if (grid) {  // (a cross batch: its two ids by (row, column))
      uint32_t res_id, sub_id;
      cross_ids_again(a.pairs, a.cols, i, res_id, sub_id);
      a.items_out[i] = uniform_item(a.u_rp, a.u_ss, a.u_ctx, res_id, sub_id);
    } else if (list) {  // (a list batch: its varying id again, the fixed one beside it)
      uint32_t res_id, sub_id;
      list_ids_again(a.pairs, a.list, a.cols, a.u_fixed, i, res_id, sub_id);
      a.items_out[i] = uniform_item(a.u_rp, a.u_ss, a.u_ctx, res_id, sub_id);
    } else {
      const unsigned long long pr = *(const GCK_GLOBAL unsigned long long*)(a.pairs + 2ull * i);
      if (shaped) a.items_out[i] = shaped_item_again(a.shape_of, a.shapes, n_shapes, i, (uint32_t)pr, (uint32_t)(pr >> 32));
      else a.items_out[i] = uniform_item(a.u_rp, a.u_ss, a.u_ctx, (uint32_t)pr, (uint32_t)(pr >> 32));
    }
  }
  if (a.coherent & kPubBySignal) {  // (closure.inc block_summary)
    const uint32_t nd = (uint32_t)__popcll(__ballot(active && !res));
    if (lane == 0 && nd) atomicAdd(&s_pub[0], nd);
    if (__ballot(ctr_touched) && lane == 0) atomicOr(&s_pub[1], 1u);
    __syncthreads();
    if (threadIdx.x == 0) block_summary(a.h_out, a.done, s_pub[0], s_pub[1], blockIdx.x);
  } else if (a.h_out) {
    // the batch's publication without a k_publish launch (closure.inc k_closure_join): the last
    // block to arrive hands the counters to the host. Coherent results: every wave's stores
    // have completed before its block arrives.
    if (a.coherent & kPubCoherent) __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (wib == 0) {
      uint32_t last = 0;
      if (lane == 0) {
        __builtin_amdgcn_s_waitcnt(0);
        last = atomicAdd(a.done, 1u) == gridDim.x - 1u;
      }
      if (__shfl(last, 0, 64)) {
        for (uint32_t k = lane; k < a.pub_words; k += 64u) a.h_out[k] = atomicExch(&a.pub[k], 0u);
        if (lane == 0) pub_seq_store(a.h_out + a.pub_words, a.seq, a.coherent);
      }
    }
  }
  const unsigned n_noroot = GCK_BUNDLE_TIMING ? (unsigned)__popcll(__ballot(active && !ua)) : 0u;
  const unsigned n_over = GCK_BUNDLE_TIMING ? (unsigned)__popcll(__ballot(why_over)) : 0u;
  const unsigned n_dirty = GCK_BUNDLE_TIMING ? (unsigned)__popcll(__ballot(why_dirty)) : 0u;
  const unsigned n_hit = GCK_BUNDLE_TIMING ? (unsigned)__popcll(__ballot(why_hit)) : 0u;
  const unsigned n_list = GCK_BUNDLE_TIMING ? (unsigned)__popcll(__ballot(used_list)) : 0u;
  const unsigned n_ext = GCK_BUNDLE_TIMING ? (unsigned)__popcll(__ballot(used_ext)) : 0u;
  if (GCK_BUNDLE_TIMING && a.timing && lane == 0) {
    unsigned long long* t = a.timing + (size_t)kLjTimingWords * (blockIdx.x * kWaves + wib);
    t[0] = t_start;
    t[1] = t_tab;
    t[2] = t_slots ? t_slots : t_tab;
    t[3] = t_dec;
    t[4] = wall_clock64();
    t[5] = n_list;
    t[6] = n_ext;
    t[7] = n_noroot;
    t[8] = n_over;
    t[9] = n_dirty;
    t[10] = n_hit;
  }
}

// Any wildcard subject in a CSR's neighbours.
__global__ void __launch_bounds__(kBlock) k_any_wildcard(const uint32_t* __restrict__ nbr, unsigned long long n,
                                                         unsigned* __restrict__ flag) {
  const unsigned long long e = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
  if (e < n && nbr[e] == kWildcard) *flag = 1u;
}

// bidir.inc k_count_subjects over the subjects rank `rank` of `world` owns, at their part_local index
// (world 1: every subject).
__global__ void __launch_bounds__(kBlock) k_count_subjects_part(const uint32_t* __restrict__ nbr,
                                                                unsigned long long n_edges, uint32_t n_sub, uint32_t rank,
                                                                uint32_t world, uint32_t* __restrict__ cnt) {
  const unsigned long long e = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_edges) return;
  const uint32_t x = nbr[e];
  if (x < n_sub && part_owner(x, world) == rank) atomicAdd(&cnt[part_local(x, world)], 1u);
}

// bidir.inc k_transpose_scatter with the rows offset by `base` (a hub's first vertex), over the
// subjects rank `rank` of `world` owns (k_count_subjects_part).
__global__ void __launch_bounds__(kBlock) k_transpose_scatter_base(const uint32_t* __restrict__ off,
                                                                   const uint32_t* __restrict__ nbr, uint32_t n_rows,
                                                                   unsigned long long n_edges, uint32_t n_sub,
                                                                   uint32_t* __restrict__ cursor,
                                                                   uint32_t* __restrict__ nbr_t, uint32_t base,
                                                                   uint32_t rank, uint32_t world) {
  __shared__ uint32_t rows[2];
  const unsigned long long e0 = (unsigned long long)blockIdx.x * kBlock;
  const unsigned long long e = e0 + threadIdx.x;
  const uint32_t o = block_edge_row(off, n_rows, n_edges, e0, e < n_edges ? e : n_edges - 1, rows);
  if (e >= n_edges) return;
  const uint32_t x = nbr[e];
  if (x < n_sub && part_owner(x, world) == rank) nbr_t[atomicAdd(&cursor[part_local(x, world)], 1u)] = base + o;
}

// The label join's variants: the kernel a HIP launch takes and its demangled name in
// libgck_kernels.co, by which the engine dispatches it into its HSA queues (aql.inc) — side by
// side, so that the two cannot name different kernels (tests/test_aql_codeobject.py reads the
// names from this text).
struct LjVariant {
  void (*kernel)(LjArgs);
  const char* aql_name;
};

// The snapshot's entry bits and slot width pick the variant, and cl: the batch's caveat tables fit
// LDS (k_label_join<..., 32, true>). (The rows in the order the launch ladder had them: the order the
// kernels are instantiated in, and so laid out in the code object.)
static const LjVariant& lj_variant(const DeviceSnapshot& ds, bool cl) {
  static const LjVariant rows[8] = {
      {k_label_join<24, 16, 32, true>, "void gck::k_label_join<24, 16u, 32u, true>(gck::LjArgs)"},
      {k_label_join<24, 32, 32, true>, "void gck::k_label_join<24, 32u, 32u, true>(gck::LjArgs)"},
      {k_label_join<32, 16, 32, true>, "void gck::k_label_join<32, 16u, 32u, true>(gck::LjArgs)"},
      {k_label_join<32, 32, 32, true>, "void gck::k_label_join<32, 32u, 32u, true>(gck::LjArgs)"},
      {k_label_join<24, 16, 32, false>, "void gck::k_label_join<24, 16u, 32u, false>(gck::LjArgs)"},
      {k_label_join<24, 32, 32, false>, "void gck::k_label_join<24, 32u, 32u, false>(gck::LjArgs)"},
      {k_label_join<32, 16, 32, false>, "void gck::k_label_join<32, 16u, 32u, false>(gck::LjArgs)"},
      {k_label_join<32, 32, 32, false>, "void gck::k_label_join<32, 32u, 32u, false>(gck::LjArgs)"}};
  return rows[(cl ? 0 : 4) + (ds.lj.bits == 24 ? 0 : 2) + (ds.lj.sw == 16 ? 0 : 1)];
}

// (32 checks per wave: 16 measured slower on configs 2 and 3 — 6.0 vs 8.3 and 8.3 vs 9.9 G
// checks/s, profiles/r04/lj_cpw/)
static uint32_t lj_blocks(uint32_t n) { return (n + 32u * kWaves - 1) / (32u * kWaves); }

// The label join over a batch through HIP; e0 / e1: the kernel's own start / stop events, or null.
static void lj_launch(const LjVariant& v, const LjArgs& j, uint32_t n, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  hipExtLaunchKernelGGL(v.kernel, dim3(lj_blocks(n)), dim3(kBlock), 0, st, e0, e1, 0, j);
  HIP_OK(hipGetLastError());
}

// The arguments that name the snapshot's join table (LjArgs::table ...).
static void lj_table_args(const DeviceSnapshot& ds, LjArgs& j) {
  j.table = ds.d_lj;
  j.n_fwd = ds.n_fwd;
  j.table_bytes = (uint32_t)((ds.lj.host.size() + 3) & ~(size_t)3);
  j.o_meta = ds.lj.o_meta;
}

// The marks of one Watch batch in one launch: a job per merged direct-grant class (its subjects'
// dirty bits) and per resource root whose own wildcard grants it changed (slot headers).
constexpr int kLjMarkJobs = 12;
struct LjMarkJob {
  const unsigned long long* keys;
  const uint8_t* ins;
  const uint8_t* found;
  uint32_t* rslot;        // null: a dirty-bits job
  const uint32_t* xlab;   // dirty-bits job: the arrow-forest labels of the CSR's row type (null: none)
  uint32_t D, r_rows, sw, x_rows;
  uint32_t wmode;         // slot job: 0 the slot overflows (deferred), 1 kLjHdrWildDirty (a root of at most
                          // two terms with a chain program), 2 kLjHdrWildDirty on an extension header only
};
struct LjMarks {
  LjMarkJob j[kLjMarkJobs];
  uint32_t start[kLjMarkJobs + 1];  // first block of each job, then the grid's size
  uint32_t n, n_users;
  uint32_t* bits;
  uint32_t* dov;  // the dirty subjects' changed objects (null: no arrow forest)
};

__global__ void __launch_bounds__(kBlock) k_lj_marks(LjMarks m) {
  uint32_t k = 0;
  while (k + 1 < m.n && blockIdx.x >= m.start[k + 1]) ++k;
  const LjMarkJob& J = m.j[k];
  const uint32_t d = (blockIdx.x - m.start[k]) * kBlock + threadIdx.x;
  if (d >= J.D || !(J.ins[d] | J.found[d])) return;
  const unsigned long long key = J.keys[d];
  const uint32_t sid = (uint32_t)key;
  if (!J.rslot) {
    if (sid >= m.n_users) return;
    if (m.dov) {  // the changed object's forest interval into the subject's list (once each)
      uint32_t* L = m.dov + (size_t)sid * kDovWords;
      const uint32_t x = (uint32_t)(key >> 32);
      if (J.xlab && x < J.x_rows) {
        const uint32_t lo = J.xlab[2 * (size_t)x], hi = J.xlab[2 * (size_t)x + 1];
        const uint32_t c = min(__hip_atomic_load(&L[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ~kDovOver, kDovPairs);
        bool seen = false;
        for (uint32_t k = 0; k < c && !seen; ++k) seen = L[2 + 2 * k] == lo && L[3 + 2 * k] == hi;
        if (!seen) {  // (two keys racing on one subject may both append it: harmless)
          const uint32_t k = atomicAdd(&L[0], 1u) & ~kDovOver;
          if (k < kDovPairs) {
            L[2 + 2 * k] = lo;
            L[3 + 2 * k] = hi;
          } else {
            atomicOr(&L[0], kDovOver);
          }
        }
      } else {  // (an object the forest does not hold, created since: every check of the subject defers)
        atomicOr(&L[0], kDovOver);
      }
    }
    atomicOr(&m.bits[sid >> 5], 1u << (sid & 31));
  } else {
    const uint32_t x = (uint32_t)(key >> 32);
    if (sid != kWildcard || x >= J.r_rows) return;
    uint32_t* h = &J.rslot[(size_t)x * J.sw];
    // (kLjHdrWildDirty is or-ed: a header already overflowed stays so; with three inline terms bit 29
    // is the third term's wildcard flag, so only an extension header carries the mark there)
    if (J.wmode == 1u || (J.wmode == 2u && (__hip_atomic_load(h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kLjHdrExt)))
      atomicOr(h, kLjHdrWildDirty);
    else
      atomicOr(h, kLjHdrOverflow);
  }
}

// Per object: does its height reach the budget under one heights array and not the other?
__global__ void __launch_bounds__(kBlock) k_deep_diff(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                      uint32_t n, uint32_t max_depth, unsigned* __restrict__ flag) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n && (a[i] >= max_depth) != (b[i] >= max_depth)) *flag = 1u;
}

// ---- the label join over a partitioned graph (partition.inc part_join_*) -----------------------
// The subject's slot lives with the subject's owner, the resource's slot with the resource's owner
// (gck_internal.hpp part_owner; the hierarchy labels are replicated). Per batch: the owner of each
// check's subject sends (check, user slot) to the owner of its resource — one all-to-all of 80-B
// records — which decides the check; an all-reduce MAX of the result bytes gives every rank every
// answer, and what no rank could decide goes to the level-synchronous loop.

constexpr uint32_t kPjRecWords = 4 + kUSlotWords;  // check index (+3 words: 16-B aligned), the subject's user slot

struct LjTab {
  const unsigned char* table;
  uint32_t n_fwd, o_meta;
};

// The label root of item `it` and its slot rows, or false.
__device__ __forceinline__ bool lj_root(const LjTab& T, const gck_item& it, LjMeta& M) {
  if (it.permission >= T.n_fwd || it.subject_relation != kEllipsis) return false;
  const uint32_t d = gptr(reinterpret_cast<const uint16_t*>(T.table))[it.permission];
  if (d == 0xFFFFu) return false;
  M = reinterpret_cast<const LjMeta*>(T.table + T.o_meta)[d];
  return it.resource_type == M.rtype && it.subject_type == M.utype && it.subject_id < M.u_rows &&
         it.resource_id < M.r_rows;
}

__device__ __forceinline__ gck_item load_item(const gck_item* items, uint32_t i) {
  uint32_t w[5];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(items + i);
  for (uint32_t q = 0; q < 5u; ++q) w[q] = gptr(src)[q];
  gck_item it;
  __builtin_memcpy(&it, w, sizeof(it));
  return it;
}

// One thread per check: a check whose subject this rank owns sends (check, user slot) to the
// owner of its resource — out region `dest` of `cap` records. A subject whose covers are a list
// (kSlotList: the list lives with the subject's owner) sends it along: the header record carries
// the number of continuation records, each with 16 cover entries (word 0 = kPjCont). Records past
// a region's end are not written; their checks stay undecided and go to the level loop (a
// reservation that straddles the end is filled with kPjCont records, which decide nothing).
constexpr uint32_t kPjCont = 0xFFFFFFFFu;  // record word 0: a continuation (or filler) record
constexpr uint32_t kPjMaxCont = 16;        // continuation records per check (256 covers)

__global__ void __launch_bounds__(kBlock) k_pj_pack(LjTab T, const gck_item* __restrict__ items, uint32_t n, uint32_t rank,
                                                    uint32_t world, uint32_t* __restrict__ out, uint32_t cap,
                                                    unsigned* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  gck_item it{};
  LjMeta M{};
  bool has = false;
  uint32_t dest = 0, n_cont = 0;
  u32x4 v[kUSlotWords / 4];
  if (i < n) {
    it = load_item(items, i);
    has = lj_root(T, it, M) && part_owner(it.subject_id, world) == rank;
    dest = has ? part_owner(it.resource_id, world) : 0u;
  }
  if (has) {
    const GCK_GLOBAL u32x4* us = (const GCK_GLOBAL u32x4*)(M.uslot + (size_t)part_local(it.subject_id, world) * kUSlotWords);
#pragma unroll
    for (uint32_t q = 0; q < kUSlotWords / 4; ++q) v[q] = us[q];
    const uint32_t w0 = v[0].x;
    if (w0 & kSlotOverflow) {
      has = false;  // (undecidable from slots: the level loop)
    } else if (w0 & kSlotList) {
      n_cont = (slot_list_count(w0) + 15u) / 16u;
      if (n_cont > kPjMaxCont) has = false;
    }
  }
  // one counter add per wave and destination for the single-record checks (every check of a rank
  // adds to the same few counters: per-lane atomics would serialise on them); per lane for the rare
  // list subjects
  const bool single = has && n_cont == 0;
  uint32_t k = 0;
  unsigned long long active = __ballot(single);
  while (active) {
    const int leader = __ffsll((long long)active) - 1;
    const uint32_t d = (uint32_t)__shfl((int)dest, leader, 64);
    const unsigned long long m = __ballot(single && dest == d);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&cnt[d], (unsigned)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader, 64);
    if (single && dest == d) k = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    active &= ~m;
  }
  if (!has) return;
  if (n_cont) k = atomicAdd(&cnt[dest], 1u + n_cont);
  GCK_GLOBAL u32x4* rec = (GCK_GLOBAL u32x4*)(out + ((size_t)dest * cap) * kPjRecWords);
  constexpr uint32_t R4 = kPjRecWords / 4;  // 16-B chunks per record
  if (k + 1 + n_cont > cap) {  // past the region's end: filler over what of it lies inside
    for (uint32_t j = k; j < cap && j < k + 1 + n_cont; ++j) rec[(size_t)j * R4] = u32x4{kPjCont, 0u, 0u, 0u};
    return;
  }
  rec[(size_t)k * R4] = u32x4{i, n_cont, 0u, 0u};
#pragma unroll
  for (uint32_t q = 0; q < kUSlotWords / 4; ++q) rec[(size_t)k * R4 + 1 + q] = v[q];
  if (n_cont) {
    const uint32_t ng = slot_list_count(v[0].x);
    const uint32_t* list = M.ulist + v[kUSlotWords / 4 - 1].w;  // (slot_list_off: the slot's last word)
    for (uint32_t c = 0; c < n_cont; ++c) {
      GCK_GLOBAL u32x4* cr = rec + (size_t)(k + 1 + c) * R4;
      cr[0] = u32x4{kPjCont, 0u, 0u, 0u};
      uint32_t w[16];
      for (uint32_t q = 0; q < 16; ++q) w[q] = 16 * c + q < ng ? gptr(list)[16 * c + q] : 0u;
      for (uint32_t q = 0; q < 4; ++q) cr[1 + q] = u32x4{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
    }
  }
}

// A subject's cover list shipped in continuation records (k_pj_pack): entry k in record k / 16.
struct LjRecCovers {
  const uint32_t* recs;  // the first continuation record
  uint32_t ng;
  __device__ __forceinline__ bool any_in(uint32_t lo, uint32_t len) const {
    for (uint32_t k = 0; k < ng; ++k)
      if (gptr(recs)[(size_t)(k / 16) * kPjRecWords + 4 + k % 16] - lo < len) return true;
    return false;
  }
};

// One thread per received record: the owner of the check's resource decides it from the user slot
// in the record and its own resource slot (sw words, at the resource's part_local index; a hub
// root's label is replicated, at its global id; labels.inc k_label_join's rules). Checks it cannot
// decide keep perm 0.
template <int BITS>
__global__ void __launch_bounds__(kBlock) k_pj_decide(LjTab T, const gck_item* __restrict__ items, uint32_t n, uint32_t sw,
                                                      uint32_t world,
                                                      const uint32_t* __restrict__ recs, uint32_t n_recs,
                                                      const unsigned* __restrict__ n_dev, uint8_t* __restrict__ perm,
                                                      int32_t* __restrict__ err) {
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= (n_dev ? min(*n_dev, n_recs) : n_recs)) return;  // n_dev: the count as the pack left it
  const GCK_GLOBAL u32x4* rec = (const GCK_GLOBAL u32x4*)(recs + (size_t)k * kPjRecWords);
  u32x4 rv[1 + kUSlotWords / 4];
#pragma unroll
  for (uint32_t q = 0; q < 1 + kUSlotWords / 4; ++q) rv[q] = rec[q];
  const uint32_t i = rv[0].x;
  if (i == kPjCont || i >= n) return;  // (a continuation or filler record)
  const uint32_t* cont = recs + ((size_t)k + 1) * kPjRecWords;
  const gck_item it = load_item(items, i);
  LjMeta M;
  if (!lj_root(T, it, M)) return;
  uint32_t uw[kUSlotWords];
#pragma unroll
  for (uint32_t q = 0; q < kUSlotWords / 4; ++q)
    uw[4 * q] = rv[1 + q].x, uw[4 * q + 1] = rv[1 + q].y, uw[4 * q + 2] = rv[1 + q].z, uw[4 * q + 3] = rv[1 + q].w;
  if (uw[0] & kSlotOverflow) return;
  bool has = false;
  uint32_t res = 0;
  // (no check contexts on a partitioned call: a caveated pair is CONDITIONAL)
  const auto cavf = [](uint32_t) { return 2u; };
  if (!M.n_terms) {  // hub root: the vertex's own interval
    const uint32_t* lab = M.rslot + 2 * (size_t)it.resource_id;
    const uint32_t hi = gptr(lab)[1];
    if (hi & kLjDeep) return;
    const uint32_t lo = gptr(lab)[0] & ~kSlotOverflow, len = hi - lo;
    if (uw[0] & kSlotList) {  // (the list came along in the continuation records)
      has = LjRecCovers{cont, slot_list_count(uw[0])}.any_in(lo, len);
    } else {
      LjInlineCovers<BITS> ci;
      slot_unpack<BITS>(uw, ci.p);
      ci.ng = uw[0];
      has = ci.any_in(lo, len);
    }
  } else {
    const uint32_t* rw = M.rslot + (size_t)part_local(it.resource_id, world) * sw;  // (this rank's slots)
    const uint32_t hdr = gptr(rw)[0];
    if (hdr & kSlotOverflow) return;
    const uint32_t* rx = (hdr & kLjHdrExt) ? M.rext + gptr(rw)[1] : nullptr;
    if (uw[0] & kSlotList) {
      const LjRecCovers cr{cont, slot_list_count(uw[0])};
      res = lj_decide_root(M, it.subject_id, hdr, rw, rx, cr, cavf);
    } else {
      LjInlineCovers<BITS> ci;
      slot_unpack<BITS>(uw, ci.p);
      ci.ng = uw[0];
      res = lj_decide_root(M, it.subject_id, hdr, rw, rx, ci, cavf);
    }
  }
  if (!M.n_terms) res = has ? (uint32_t)GCK_PERM_HAS : (uint32_t)GCK_PERM_NO;
  perm[i] = (uint8_t)res;
  err[i] = GCK_ITEM_OK;
}

// Leftover compaction in batch order without a host round trip per step: per-block counts of the
// undecided checks, one block scanning them (the total also goes to `total`), then each block
// places its own in order.
__global__ void __launch_bounds__(kBlock) k_pj_bcount(const uint8_t* __restrict__ perm, uint32_t n,
                                                      uint32_t* __restrict__ bc) {
  __shared__ uint32_t s[kWaves];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const unsigned long long m = __ballot(i < n && perm[i] == 0);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < kWaves; ++w) t += s[w];
    bc[blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(kBlock) k_pj_bscan(uint32_t* __restrict__ bc, uint32_t nb, uint32_t* __restrict__ total) {
  if (threadIdx.x != 0) return;
  uint32_t run = 0;  // (a few hundred to a few thousand blocks: one lane is enough)
  for (uint32_t b = 0; b < nb; ++b) {
    const uint32_t c = bc[b];
    bc[b] = run;
    run += c;
  }
  *total = run;
}

__global__ void __launch_bounds__(kBlock) k_pj_place(const gck_item* __restrict__ items, const uint8_t* __restrict__ perm,
                                                     uint32_t n, const uint32_t* __restrict__ boff,
                                                     uint32_t* __restrict__ idx, gck_item* __restrict__ left) {
  __shared__ uint32_t s[kWaves];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool f = i < n && perm[i] == 0;
  const unsigned long long m = __ballot(f);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s[wv] = (uint32_t)__popcll(m);
  __syncthreads();
  if (!f) return;
  uint32_t at = boff[blockIdx.x];
  for (int w = 0; w < wv; ++w) at += s[w];
  at += (uint32_t)__popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
  idx[at] = i;
  left[at] = items[i];
}
