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
// Per dirty subject (DeviceSnapshot::lj_dov), two lines: word 0 the appends made (low 31 bits) |
// kDovOver once one did not fit, word 1 unused, then kDovPairs (lo, hi) arrow-forest intervals of
// the objects whose direct grants of the subject changed since the tables were built — pairs 0-6
// in the first line, 7-14 in the second.
constexpr uint32_t kDovWords = 32, kDovPairs = 15, kDovOver = 0x80000000u;

// The chain program of a root (build_labels lj_chain_of): per term, the direct-user CSR classes its
// flattening reads at each depth of the resource's arrow-forest chain (R, R's parent, ...), so that a
// dirty subject's check whose overlay hits (a changed grant on the chain) is decided in the join
// from the current revision's rows instead of going to the bundles. A level is one set of schema
// nodes on one object; the levels of a term form a path that may loop (a folder's parent->view
// reaches folder#view again).
constexpr uint32_t kLjChainCls = 8, kLjChainLvls = 8, kLjChainDepth = 64;
constexpr uint8_t kLjChainEnd = 0xFF;
struct LjChainLvl {
  uint32_t af_base;             // forest index of object 0 of the level's type (DeviceSnapshot::lj_af_base)
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
  // the resources' (pre, end) in the arrow forest (DeviceSnapshot::lj_af; null: none): a dirty
  // subject's check stays with the slots unless a changed object's interval holds pre(R)
  const uint32_t* apre;
  // the chain program (null: a dirty subject's overlay hit defers the check)
  const LjChain* chain;
};
static_assert(sizeof(LjMeta) == 64, "LjMeta layout");

struct LjArgs {
  const gck_item* items;
  uint32_t n;
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
  // the call's check contexts (a device copy of the batch's Ctx: caveat outcomes, the lazy
  // evaluation's request set, cav_flag), or null: a caveated pair is then CONDITIONAL
  const Ctx* cx;
  // subjects whose direct grants changed since the tables were built (a bit each; null: none):
  // their checks go to the bundles (labels.inc lj_dirty_path)
  const uint32_t* dirty;
  // the caveat instances and the dense outcome table's rows (k_label_join<..., CL>: staged in LDS)
  uint32_t cav_n, cav_rows;
  // host items read in place: the request check of their context slots (CjArgs::bad_slot)
  unsigned* bad_slot;
  uint32_t slot_limit;
  // the dirty subjects' changed objects (kDovWords per subject; null: a dirty subject defers)
  const uint32_t* dov;
  unsigned long long* timing;  // GCK_DEBUG_TIMING (TIMING=1 builds): kLjTimingWords per wave
  // a uniform batch (closure.inc CjArgs::pairs)
  const uint32_t* pairs;
  unsigned long long* out_packed;
  gck_item* items_out;
  uint32_t u_rp, u_ss, u_ctx;
  // the chain walk of a dirty subject's overlay hit (LjMeta::chain): the current revision's CSRs
  // and the forest's parent edges (DeviceSnapshot::lj_afp: tupleset CSR << 32 | parent's index)
  const DevCSR* csrs;
  const unsigned long long* afp;
  uint32_t n_csrs, afp_n;  // (the walk's bounds: every index it reads is checked against them)
  const uint8_t* cav_static;  // per caveat instance its outcome under its stored context (the walk)
  const uint32_t* anc;        // per forest vertex its ancestors (kAncWords, DeviceSnapshot::lj_anc; null: none)
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

// Per forest vertex one 64-B line (DeviceSnapshot::lj_anc): word 0 the number of its ancestors
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
  const uint32_t* lp = list ? M.ulist + uw[1] : nullptr;
  const uint32_t ng = list ? uw[0] & ~(kSlotList | kSlotOverflow) : uw[0];
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
  const uint32_t* lp = list ? M.ulist + uw[1] : nullptr;
  const uint32_t ng = list ? uw[0] & ~(kSlotList | kSlotOverflow) : uw[0];
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
  const bool uni = a.pairs != nullptr;  // a uniform batch (a scalar branch)
  const uint32_t item_bytes = w0 < a.n ? min(CPW, a.n - w0) * 20u : 0u;
  const unsigned char* ibase = reinterpret_cast<const unsigned char*>(a.items) + (size_t)w0 * 20u;
  const bool items_fast = !uni && ((uintptr_t)a.items & 15u) == 0 && item_bytes == CPW * 20u;
  u32x4 item_chunk{0u, 0u, 0u, 0u};
  if (items_fast && (threadIdx.x & 63u) < CPW * 20u / 16u)
    item_chunk = *(const GCK_GLOBAL u32x4*)(ibase + (threadIdx.x & 63u) * 16u);
  if (uni && (threadIdx.x & 63u) < CPW && w0 + (threadIdx.x & 63u) < a.n) {  // (a uniform batch: the lane's pair)
    const unsigned long long pr = *(const GCK_GLOBAL unsigned long long*)(a.pairs + 2ull * (w0 + (threadIdx.x & 63u)));
    item_chunk.x = (uint32_t)pr;
    item_chunk.y = (uint32_t)(pr >> 32);
  }
  for (uint32_t k = threadIdx.x; k < a.table_bytes / 4; k += kBlock)
    reinterpret_cast<uint32_t*>(s_tab)[k] = gptr(reinterpret_cast<const uint32_t*>(a.table))[k];
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
  const unsigned long long t_tab = (GCK_BUNDLE_TIMING && a.timing) ? wall_clock64() : 0ull;
  const uint16_t* root = reinterpret_cast<const uint16_t*>(s_tab);
  const LjMeta* meta = reinterpret_cast<const LjMeta*>(s_tab + a.o_meta);
  const int wib = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t* const stage = s_stage[wib];
  const uint32_t i = w0 + (uint32_t)lane;
  const bool active = (uint32_t)lane < CPW && i < a.n;
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
    it = uniform_item(a.u_rp, a.u_ss, a.u_ctx, item_chunk.x, item_chunk.y);
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
            has = LjListCovers{M.ulist + uw[1], uw[0] & ~(kSlotList | kSlotOverflow)}.any_in(lo, len);
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
          LjListCovers cl{M.ulist + uw[1], uw[0] & ~(kSlotList | kSlotOverflow)};
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
      LjListCovers cl{M3.ulist + uw[1], uw[0] & ~(kSlotList | kSlotOverflow)};
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
    const unsigned long long pr = *(const GCK_GLOBAL unsigned long long*)(a.pairs + 2ull * i);
    a.items_out[i] = uniform_item(a.u_rp, a.u_ss, a.u_ctx, (uint32_t)pr, (uint32_t)(pr >> 32));
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
  return rows[(cl ? 0 : 4) + (ds.lj_bits == 24 ? 0 : 2) + (ds.lj_sw == 16 ? 0 : 1)];
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
  j.table_bytes = (uint32_t)((ds.lj_host.size() + 3) & ~(size_t)3);
  j.o_meta = ds.lj_o_meta;
}

// ---- host side: hubs, hierarchy labels, user slots, flattened resource slots --------------------

// Tree labels and covers of a DAG given as parents per vertex (the same construction as
// bidir.inc build_ancestors, over any vertex set): lab[2v] = pre(v) | overflow << 31,
// lab[2v + 1] = end(v), cov_off / cov_pre the covers' preorder numbers. False on a cycle.
static bool hier_labels(uint32_t n, const std::vector<uint32_t>& poff, const std::vector<uint32_t>& pnbr,
                        const std::vector<uint32_t>& coff_all, const std::vector<uint32_t>& cnbr_all,
                        std::vector<uint32_t>& lab, std::vector<uint32_t>& cov_off, std::vector<uint32_t>& cov_pre) {
  TopoLevels T;
  if (!topo_levels(n, poff, coff_all.data(), cnbr_all.data(), T)) return false;
  tree_labels(n, poff, pnbr, T, kLjCoverMax, host_threads(), lab, cov_off, cov_pre);
  return true;
}

// Strongly connected components of the hierarchy (iterative Tarjan over the child lists):
// comp[v] in [0, n_comp). Vertices of one component reach each other, so they share their upward
// closure; the labels are built over the condensed DAG. (Checks whose resource reaches a cycle sit
// at the depth budget and are deferred by the height guard; everything else stays exact.)
// `trivial`: vertices known to lie on no cycle (Kahn's order reached them: their parents all
// came first), each its own component without a visit — a remaining vertex's children are
// remaining too (an edge into a Kahn-ordered vertex would have held it back), so Tarjan runs over
// the remaining ones alone: the cycles and what lies below them.
static uint32_t hier_scc(uint32_t n, const std::vector<uint32_t>& coff, const std::vector<uint32_t>& cnbr,
                         const std::vector<char>& trivial, std::vector<uint32_t>& comp) {
  constexpr uint32_t kUnset = 0xFFFFFFFFu;
  std::vector<uint32_t> index(n, kUnset), low(n, 0), stack, it_pos(n, 0), call;
  std::vector<char> on(n, 0);
  comp.assign(n, kUnset);
  uint32_t next_index = 0, n_comp = 0;
  for (uint32_t s = 0; s < n; ++s)
    if (trivial[s]) index[s] = next_index++, comp[s] = n_comp++;
  for (uint32_t s = 0; s < n; ++s) {
    if (index[s] != kUnset) continue;
    call.push_back(s);
    index[s] = low[s] = next_index++;
    stack.push_back(s);
    on[s] = 1;
    it_pos[s] = coff[s];
    while (!call.empty()) {
      const uint32_t v = call.back();
      if (it_pos[v] < coff[v + 1]) {
        const uint32_t w = cnbr[it_pos[v]++];
        if (index[w] == kUnset) {
          index[w] = low[w] = next_index++;
          stack.push_back(w);
          on[w] = 1;
          it_pos[w] = coff[w];
          call.push_back(w);
        } else if (on[w]) {
          low[v] = std::min(low[v], index[w]);
        }
        continue;
      }
      call.pop_back();
      if (!call.empty()) low[call.back()] = std::min(low[call.back()], low[v]);
      if (low[v] == index[v]) {
        for (;;) {
          const uint32_t w = stack.back();
          stack.pop_back();
          on[w] = 0;
          comp[w] = n_comp;
          if (w == v) break;
        }
        ++n_comp;
      }
    }
  }
  return n_comp;
}

// Tree labels and covers of any hierarchy (cycles condensed): per vertex lab[2v] / lab[2v + 1]
// and its cover (cov_off / cov_pre), those of its component.
static void hier_labels_any(uint32_t n, const std::vector<uint32_t>& poff, const std::vector<uint32_t>& pnbr,
                            const std::vector<uint32_t>& coff, const std::vector<uint32_t>& cnbr, std::vector<uint32_t>& lab,
                            std::vector<uint32_t>& cov_off, std::vector<uint32_t>& cov_pre, uint32_t& n_cyclic) {
  n_cyclic = 0;
  PhaseClock pc("hier");
  if (hier_labels(n, poff, pnbr, coff, cnbr, lab, cov_off, cov_pre)) return;
  pc.mark("acyclic_try");
  std::vector<char> trivial(n, 0);
  {  // Kahn's order over the whole hierarchy: what it reaches lies on no cycle
    std::vector<uint32_t> indeg(n), q;
    q.reserve(n);
    for (uint32_t v = 0; v < n; ++v)
      if (!(indeg[v] = poff[v + 1] - poff[v])) q.push_back(v);
    for (size_t qi = 0; qi < q.size(); ++qi) {
      trivial[q[qi]] = 1;
      for (uint32_t k = coff[q[qi]]; k < coff[q[qi] + 1]; ++k)
        if (--indeg[cnbr[k]] == 0) q.push_back(cnbr[k]);
    }
  }
  std::vector<uint32_t> comp;
  const uint32_t nc = hier_scc(n, coff, cnbr, trivial, comp);
  pc.mark("scc");
  std::vector<uint32_t> csize(nc, 0);
  for (uint32_t v = 0; v < n; ++v) ++csize[comp[v]];
  for (uint32_t v = 0; v < n; ++v) n_cyclic += csize[comp[v]] > 1 ? 1u : 0u;
  // the condensed DAG (parent comp -> child comp, deduplicated): the edges bucketed by parent
  // component (a counting sort), each bucket sorted and deduplicated in parallel, then the
  // parents lists from the children lists
  std::vector<uint32_t> bo((size_t)nc + 1, 0), bk;
  for (uint32_t v = 0; v < n; ++v)
    for (uint32_t k = coff[v]; k < coff[v + 1]; ++k)
      if (comp[v] != comp[cnbr[k]]) ++bo[comp[v] + 1];
  for (uint32_t c = 0; c < nc; ++c) bo[c + 1] += bo[c];
  bk.resize(bo[nc]);
  {
    std::vector<uint32_t> at(bo.begin(), bo.end() - 1);
    for (uint32_t v = 0; v < n; ++v)
      for (uint32_t k = coff[v]; k < coff[v + 1]; ++k)
        if (comp[v] != comp[cnbr[k]]) bk[at[comp[v]]++] = comp[cnbr[k]];
  }
  std::vector<uint32_t> blen(nc, 0);
  parallel_chunks(nc, host_threads(), [&](unsigned, size_t lo, size_t hi) {
    for (size_t c = lo; c < hi; ++c) {
      std::sort(bk.begin() + bo[c], bk.begin() + bo[c + 1]);
      blen[c] = (uint32_t)(std::unique(bk.begin() + bo[c], bk.begin() + bo[c + 1]) - (bk.begin() + bo[c]));
    }
  });
  std::vector<uint32_t> qcoff((size_t)nc + 1, 0);
  for (uint32_t c = 0; c < nc; ++c) qcoff[c + 1] = qcoff[c] + blen[c];
  std::vector<uint32_t> qcnbr(qcoff[nc]), qpoff((size_t)nc + 1, 0), qpnbr(qcoff[nc]);
  for (uint32_t c = 0; c < nc; ++c) {
    std::copy(bk.begin() + bo[c], bk.begin() + bo[c] + blen[c], qcnbr.begin() + qcoff[c]);
    for (uint32_t k = 0; k < blen[c]; ++k) ++qpoff[bk[bo[c] + k] + 1];
  }
  for (uint32_t c = 0; c < nc; ++c) qpoff[c + 1] += qpoff[c];
  {
    std::vector<uint32_t> pa(qpoff.begin(), qpoff.end() - 1);
    for (uint32_t c = 0; c < nc; ++c)  // (parents in ascending order, as the sorted edge list gave them)
      for (uint32_t k = qcoff[c]; k < qcoff[c + 1]; ++k) qpnbr[pa[qcnbr[k]]++] = c;
  }
  pc.mark("condense");
  std::vector<uint32_t> clab, ccoff, ccpre;
  if (!hier_labels(nc, qpoff, qpnbr, qcoff, qcnbr, clab, ccoff, ccpre))
    throw Error(GCK_E_DEVICE, "engine invariant violated: condensed hierarchy is cyclic");
  lab.assign(2 * (size_t)n, 0);
  cov_off.assign((size_t)n + 1, 0);
  const unsigned nt = host_threads();
  parallel_chunks(n, nt, [&](unsigned, size_t lo, size_t hi) {
    for (size_t v = lo; v < hi; ++v) {
      const uint32_t c = comp[v];
      lab[2 * v] = clab[2 * (size_t)c];
      lab[2 * v + 1] = clab[2 * (size_t)c + 1];
      cov_off[v + 1] = ccoff[c + 1] - ccoff[c];
    }
  });
  for (uint32_t v = 0; v < n; ++v) cov_off[v + 1] += cov_off[v];
  cov_pre.resize(cov_off[n]);
  parallel_chunks(n, nt, [&](unsigned, size_t lo, size_t hi) {
    for (size_t v = lo; v < hi; ++v)
      std::copy(ccpre.begin() + ccoff[comp[v]], ccpre.begin() + ccoff[comp[v] + 1], cov_pre.begin() + cov_off[v]);
  });
  pc.mark("labels_expand");
}

namespace {

struct HostRows {  // a host copy of one CSR of the snapshot
  std::vector<uint32_t> off, nbr;
  std::vector<uint32_t> cav;  // ext CSRs: caveat instance and expiry per edge
  std::vector<int64_t> exp;
  uint32_t n_rows = 0;
};

// One flattened term of one resource: users reached without entering a hub, hub vertices entered,
// a wildcard.
struct Flat {
  std::vector<uint32_t> D, V;
  std::vector<uint32_t> C;  // (user | kLjCav, instance) pairs: reached only through a partial caveat
  bool wild = false, over = false;
};

struct LabelPlan {
  uint32_t p;                    // the root (a permission node, or a hub: no terms)
  std::vector<uint32_t> terms;   // operand nodes
  uint8_t neg = 0;
  bool cav = false;              // a term reads caveated relationships (the caveat plane)
  uint32_t sw_need = 16;         // slot words the sample asked for
};

}  // namespace

// Hubs of a node program (over its forward nodes [0, nf)): targets of usersets and arrows that are
// unions of stored subjects and computed usersets, whose usersets point at hubs again, with no
// caveated / expiring edge (`ext(item index)`). loc[h]: the nodes of hub h on its own object.
template <class Ext>
static void find_hubs(const std::vector<DevNode>& nodes, const std::vector<DevItem>& items, uint32_t nf, Ext&& ext,
                      std::vector<char>& hub, std::vector<std::vector<uint32_t>>& loc) {
  std::vector<char> target(nf, 0);
  hub.assign(nf, 0);
  loc.assign(nf, {});
  for (uint32_t n = 0; n < nf; ++n)
    for (uint32_t k = 0; k < nodes[n].count; ++k) {
      const DevItem& it = items[nodes[n].first + k];
      if ((it.kind == IT_KIND && it.srel != kEllipsis) || it.kind == IT_ARROW)
        if (it.target != kNoNode && it.target < nf) target[it.target] = 1;
    }
  for (uint32_t h = 0; h < nf; ++h) {
    if (!target[h]) continue;
    std::vector<uint32_t> stack{h}, out;
    std::vector<char> seen(nf, 0);
    seen[h] = 1;
    bool ok = true;
    while (!stack.empty() && ok) {
      const uint32_t n = stack.back();
      stack.pop_back();
      out.push_back(n);
      const DevNode& nd = nodes[n];
      if (nd.kind != NK_RELATION && nd.kind != NK_UNION && nd.kind != NK_NIL) ok = false;
      for (uint32_t k = 0; k < nd.count && ok; ++k) {
        const DevItem& it = items[nd.first + k];
        if (nd.kind == NK_UNION) {
          if (it.kind != IT_COMPUTED || it.target >= nf) ok = false;
          else if (!seen[it.target]) seen[it.target] = 1, stack.push_back(it.target);
        } else if (it.kind != IT_KIND || ext(nd.first + k)) {
          ok = false;
        }
      }
    }
    if (ok) {
      hub[h] = 1;
      loc[h] = std::move(out);
    }
  }
  for (bool changed = true; changed;) {  // a hub's usersets must point at hubs
    changed = false;
    for (uint32_t h = 0; h < nf; ++h) {
      if (!hub[h]) continue;
      for (uint32_t n : loc[h])
        for (uint32_t k = 0; k < nodes[n].count && hub[h]; ++k) {
          const DevItem& it = items[nodes[n].first + k];
          if (nodes[n].kind == NK_RELATION && it.srel != kEllipsis && (it.target >= nf || !hub[it.target])) {
            hub[h] = 0;
            changed = true;
          }
        }
    }
  }
}

// The ingest rules of a partitioned graph (SURVEY §8e; engine.hpp part_keep), from the schema
// alone, so that every rank filters the export stream (client/client.go:472-499) and the Watch
// stream the same way: the hubs a label join can meet are those of the schema whose relations
// allow no caveat or expiration; the relations of those hubs are the hierarchy — their userset
// (and wildcard) tuples are replicated on every rank, their direct-subject tuples are kept also by
// the subject's owner (the subject side of the join, the user slots).
void partition_rules(Engine& e) {
  e.part_hub_node.clear();
  e.part_hub_rel.clear();
  e.part_sub_node.clear();
  if (!e.schema) return;
  const Schema& sc = *e.schema;
  const uint32_t nf = (uint32_t)sc.nodes.size();
  auto ext = [&](uint32_t i) {
    const DevItem& it = sc.items[i];
    const uint16_t rel = sc.item_rel[i];
    if (rel >= sc.rels.size()) return true;
    for (const Allowed& a : sc.rels[rel].allowed)
      if (a.stype == it.stype && a.srel == it.srel && (!a.caveat.empty() || a.expiration)) return true;
    return false;
  };
  std::vector<char> hub;
  std::vector<std::vector<uint32_t>> loc;
  find_hubs(sc.nodes, sc.items, nf, ext, hub, loc);
  // A hub relation's direct tuples live with their subjects' owners, which is right only if every
  // node that reads its rows is one of the hubs' nodes (routed there, partition.inc part_dest). A
  // hub whose relation is also read elsewhere — e.g. as an arrow's tupleset by a permission outside
  // the hub — is no hub of the partition (its rows stay with their objects' owners, its roots go to
  // the level loop); dropping one changes which nodes are hub nodes, so repeat until none is read
  // from outside.
  for (bool changed = true; changed;) {
    changed = false;
    e.part_hub_rel.assign(sc.rels.size(), 0);
    e.part_sub_node.assign(nf, 0);
    for (uint32_t h = 0; h < nf; ++h)
      if (hub[h])
        for (uint32_t n : loc[h]) {
          e.part_sub_node[n] = 1;
          if (n < sc.rels.size() && sc.nodes[n].kind == NK_RELATION) e.part_hub_rel[n] = 1;
        }
    std::vector<char> bad(sc.rels.size(), 0);
    for (uint32_t n = 0; n < nf; ++n) {
      if (e.part_sub_node[n]) continue;
      for (uint32_t k = 0; k < sc.nodes[n].count; ++k) {
        const uint32_t i = sc.nodes[n].first + k;
        const uint8_t kind = sc.items[i].kind;
        if (kind != IT_KIND && kind != IT_ARROW) continue;
        const uint16_t rel = sc.item_rel[i];
        if (rel < bad.size() && e.part_hub_rel[rel]) bad[rel] = 1;
      }
    }
    for (uint32_t h = 0; h < nf; ++h) {
      if (!hub[h]) continue;
      for (uint32_t n : loc[h])
        if (n < bad.size() && bad[n]) {
          hub[h] = 0;
          changed = true;
          break;
        }
    }
  }
  e.part_hub_node.assign(hub.begin(), hub.end());
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

// May a Watch batch keep the current label tables although some of their CSRs changed? When every
// changed one is a direct-grant CSR (`dkey`, the users listed in resource slots) that the batch
// merged (Engine::delta_hint), no wildcard grant changed, no root's resource crossed the depth
// budget: the checks of the subjects whose grants
// changed then go to the wave bundles (k_label_join reads the dirty set), everything else the
// tables answer as before — a 0.1 % churn of direct grants (BASELINE config 5) rebuilds nothing.
// Not on a partitioned graph (its slots live on several ranks).
// `own_only`: the direct-grant CSRs every root reads only on its resource's own object (a changed
// wildcard grant there changes that resource alone). `why`: the reason a rebuild is needed.
static bool lj_dirty_path(const Engine& e, const DeviceSnapshot& ds, const std::vector<uint64_t>& dkey,
                          const std::vector<const uint32_t*>& hkey, uint32_t max_depth,
                          const std::vector<uint32_t>& own_only, const std::vector<uint32_t>& hroots,
                          const char*& why) {
  const DeviceSnapshot& old = *e.dev;
  why = "not a Watch batch";
  if (!e.delta_hint || e.part_world > 1) return false;
  why = "other grant CSRs";
  if (old.lj_dkey.size() != dkey.size() || old.lj_hgt.size() != hkey.size()) return false;
  uint64_t marks = 0;
  for (size_t q = 0; q < dkey.size(); q += 4) {
    if (old.lj_dkey[q] != dkey[q]) return false;  // (another CSR)
    if (old.lj_dkey[q + 1] == dkey[q + 1] && old.lj_dkey[q + 2] == dkey[q + 2]) continue;
    const DeltaHint::Fwd* f = nullptr;
    for (const DeltaHint::Fwd& x : e.delta_hint->fwd)
      if ((uint64_t)(uintptr_t)x.nbr == dkey[q + 1]) f = &x;
    why = "a grant CSR the batch did not merge";
    if (!f) return false;
    why = "a wildcard grant read beyond its own object";
    if (f->wild && !std::binary_search(own_only.begin(), own_only.end(), (uint32_t)dkey[q])) return false;
    marks += f->D;
  }
  // (No rebuild for dirtiness: a dirty subject's checks cost the bundles' time, as without the
  // tables, while a rebuild — 0.45 s for config 2's 2.2M resources — would not pay for itself in
  // ten thousand batches.)
  (void)marks;
  // heights: a changed array must leave every resource on the same side of the budget
  for (size_t k = 0; k < hkey.size(); ++k) {
    if (old.lj_hgt[k] == hkey[k]) continue;
    if (!old.lj_hgt[k] || !hkey[k]) return false;
    const uint32_t p = hroots[k];  // (no resource of the root near the budget before or after)
    if (p < old.hmax.size() && p < ds.hmax.size() && old.hmax[p] < max_depth && ds.hmax[p] < max_depth) continue;
    uint32_t n = 0;
    for (uint32_t p = 0; p < ds.hgt.size(); ++p)
      if (ds.hgt[p] == hkey[k]) n = ds.hcount[p];
    uint32_t n_old = 0;
    for (uint32_t p = 0; p < old.hgt.size(); ++p)
      if (old.hgt[p] == old.lj_hgt[k]) n_old = old.hcount[p];
    why = "heights";
    if (n != n_old) return false;
    std::vector<void*> tmp;
    unsigned hv = 0;
    try {
      unsigned* flag = dalloc<unsigned>(tmp, 1);
      HIP_OK(hipMemset(flag, 0, 4));
      if (n) hipLaunchKernelGGL(k_deep_diff, dim3(grid_for(n)), dim3(kBlock), 0, 0, old.lj_hgt[k], hkey[k], n, max_depth, flag);
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemcpy(&hv, flag, 4, hipMemcpyDeviceToHost));
    } catch (...) {
      free_list(tmp);
      throw;
    }
    free_list(tmp);
    if (hv) return false;
  }
  return true;
}

// Marks the subjects whose direct grants the batch changed (lj_dirty_path held): the dirty set is
// shared with the current snapshot — bits are only ever set, and a check of the current revision
// that sees one goes to the bundles, which answer it from that revision's CSRs.
static void lj_mark_dirty(Engine& e, DeviceSnapshot& ds, const std::vector<uint64_t>& dkey,
                          const std::map<uint32_t, std::vector<uint32_t>>& own_roots) {
  const DeviceSnapshot& old = *e.dev;
  const uint32_t n_users = ds.lj_users;
  if (!ds.lj_dirty) {
    const size_t bytes = ((size_t)n_users / 32 + 1) * 4;
    uint32_t* q = slot_alloc(ds, bytes);
    HIP_OK(hipMemset(q, 0, bytes));
    ds.lj_ptrs.push_back(q);
    ds.lj_bytes += bytes;
    ds.bytes += bytes;
    ds.lj_dirty = q;
  }
  if (ds.lj_af && !ds.lj_dov) {  // the changed objects of each dirty subject (kDovWords per subject)
    const size_t bytes = ((size_t)n_users + 1) * kDovWords * 4;
    uint32_t* q = slot_alloc(ds, bytes);
    HIP_OK(hipMemset(q, 0, bytes));
    ds.lj_ptrs.push_back(q);
    ds.lj_bytes += bytes;
    ds.bytes += bytes;
    ds.lj_dov = q;
  }
  LjMarks m{};
  m.n_users = n_users;
  m.bits = ds.lj_dirty;
  m.dov = ds.lj_dov;
  auto flush = [&]() {
    if (!m.n) return;
    hipLaunchKernelGGL(k_lj_marks, dim3(m.start[m.n]), dim3(kBlock), 0, 0, m);
    m.n = 0;
  };
  auto add = [&](const DeltaHint::Fwd& f, uint32_t* rslot, uint32_t r_rows, const uint32_t* xlab, uint32_t x_rows,
                 uint32_t wmode) {
    if (m.n == (uint32_t)kLjMarkJobs) flush();
    LjMarkJob& J = m.j[m.n];
    J = LjMarkJob{f.keys, f.ins, f.found, rslot, xlab, f.D, r_rows, ds.lj_sw, x_rows, wmode};
    m.start[m.n + 1] = m.start[m.n] + grid_for(f.D);
    ++m.n;
  };
  // the forest labels of a direct-grant CSR's rows (its relation's resource type)
  auto xlab_of = [&](uint32_t c, uint32_t& rows) -> const uint32_t* {
    rows = 0;
    if (!ds.lj_af) return nullptr;
    for (auto& [cc, t] : ds.lj_dtype)
      if (cc == c && t < ds.lj_af_base.size() && ds.lj_af_base[t] != kNone) {
        rows = ds.lj_af_rows[t];
        return ds.lj_af + 2 * (size_t)ds.lj_af_base[t];
      }
    return nullptr;
  };
  for (size_t q = 0; q < dkey.size(); q += 4) {
    if (old.lj_dkey[q + 1] == dkey[q + 1] && old.lj_dkey[q + 2] == dkey[q + 2]) continue;
    uint32_t x_rows = 0;
    const uint32_t* xlab = xlab_of((uint32_t)dkey[q], x_rows);
    for (const DeltaHint::Fwd& f : e.delta_hint->fwd)
      if ((uint64_t)(uintptr_t)f.nbr == dkey[q + 1] && f.D) {
        add(f, nullptr, 0u, xlab, x_rows, 0u);
        ds.lj_dirty_n += f.D;
        auto ro = own_roots.find((uint32_t)dkey[q]);
        if (f.wild && ro != own_roots.end())  // (lj_dirty_path: read on the resource's own object only)
          for (uint32_t p : ro->second) {
            const uint16_t d = reinterpret_cast<const uint16_t*>(ds.lj_host.data())[p];
            if (d == 0xFFFFu) continue;
            LjMeta M;
            std::memcpy(&M, ds.lj_host.data() + ds.lj_o_meta + (size_t)d * sizeof(LjMeta), sizeof(LjMeta));
            // (a chain program: the walk reads the wildcard's current grants, lj_redecide)
            const uint32_t wmode = !M.chain || !ds.lj_afp ? 0u : M.n_terms < 3u ? 1u : 2u;
            if (M.n_terms) add(f, const_cast<uint32_t*>(M.rslot), M.r_rows, nullptr, 0u, wmode);
          }
      }
  }
  flush();
  // (no synchronisation: the marks are ordered on the null stream before the publication, and
  // the delta arena they read is rewritten only by the next batch, behind them on that stream)
  HIP_OK(hipGetLastError());
}

// Builds the label join's tables for the snapshot into ds (lj_*), or nothing when no permission
// qualifies. Runs after build_bidir (heights are known; the closure join, when the snapshot has
// one of its roots, keeps the stage: the two are not combined).
static void build_labels(Engine& e, DeviceSnapshot& ds, const std::vector<DevNode>& nodes,
                         const std::vector<DevItem>& items, const std::vector<DevCSR>& table,
                         const std::vector<CsrInfo>& info) {
  ds.lj_host.clear();
  ds.lj_sw = 0;
  ds.lj_preferred = false;
  ds.lj_cav = false;
  if (e.cfg.flags & (GCK_FLAG_NO_LABELS | GCK_FLAG_NO_SLOTS)) return;
  // a partitioned graph (world > 1) holds this rank's rows and the replicated hub hierarchy: it
  // builds the slots of the subjects and resources it owns, indexed by part_local (the resource
  // side flattens within its own rows and the hubs, and defers a resource whose walk leaves them)
  const uint32_t P = e.part_world, prank = e.part_rank;
  PhaseClock pc("labels");
  const Schema& sc = *e.schema;
  const uint32_t nf = ds.n_fwd;
  const uint32_t R = (uint32_t)sc.rels.size();
  const uint32_t max_depth = e.cfg.max_depth ? e.cfg.max_depth : 50;
  auto count_of = [&](uint32_t type) { return e.interner[type].count; };
  auto ext_edges = [&](const DevItem& it) { return it.csr_ext != kNone && info[it.csr_ext].n_edges > 0; };
  auto has_rows = [&](uint32_t c) { return c != kNone && info[c].n_edges > 0; };
  // 1. hubs: targets of usersets and arrows that are unions of stored subjects and usersets of hubs
  std::vector<char> hub;
  std::vector<std::vector<uint32_t>> loc;  // the hub's nodes on its own object (computed usersets)
  find_hubs(nodes, items, nf, [&](uint32_t i) { return ext_edges(items[i]); }, hub, loc);
  if (e.part_world > 1)  // a partitioned graph replicates the hierarchy of the schema's hubs only
    for (uint32_t h = 0; h < nf; ++h) hub[h] &= h < e.part_hub_node.size() ? e.part_hub_node[h] : 0;
  // the subject type: the most common direct subject type of the stored relations
  std::vector<uint64_t> by_type(sc.types.size(), 0);
  for (uint32_t n = 0; n < nf; ++n)
    if (nodes[n].kind == NK_RELATION)
      for (uint32_t k = 0; k < nodes[n].count; ++k) {
        const DevItem& it = items[nodes[n].first + k];
        if (it.kind == IT_KIND && it.srel == kEllipsis && it.csr_plain != kNone) by_type[it.stype] += info[it.csr_plain].n_edges;
      }
  const uint32_t U = (uint32_t)(std::max_element(by_type.begin(), by_type.end()) - by_type.begin());
  if (by_type.empty() || by_type[U] == 0) return;
  // 2. roots: permissions whose operands flatten (unions, computed usersets, arrows, stored
  //    relations; hubs end a path)
  std::vector<uint32_t> dfeed;  // CSRs of direct subjects: they feed only the resource slots' user lists
  std::vector<std::pair<uint32_t, uint16_t>> dfeed_type;  // ... and the type of their rows
  auto flattenable = [&](uint32_t t, std::vector<uint32_t>& csrs, std::vector<uint32_t>& hubs_hit, bool& cav) {
    std::vector<uint32_t> stack{t};
    std::vector<char> seen(nf, 0);
    seen[t] = 1;
    while (!stack.empty()) {
      const uint32_t n = stack.back();
      stack.pop_back();
      if (hub[n]) {
        hubs_hit.push_back(n);
        continue;
      }
      const DevNode& nd = nodes[n];
      if (nd.kind == NK_NIL) continue;
      if (nd.kind != NK_RELATION && nd.kind != NK_UNION) return false;
      for (uint32_t k = 0; k < nd.count; ++k) {
        const DevItem& it = items[nd.first + k];
        uint32_t next = kNone;
        if (nd.kind == NK_RELATION) {
          if (it.kind != IT_KIND) return false;
          if (ext_edges(it)) {
            // caveated (or expiring) relationships to direct subjects: the caveat plane of the
            // slots; through a userset they would condition a whole hub: not flattened
            if (it.srel != kEllipsis) return false;
            csrs.push_back(it.csr_ext);
            dfeed.push_back(it.csr_ext);
            dfeed_type.push_back({it.csr_ext, nd.type});
            cav = true;
          }
          if (has_rows(it.csr_plain)) {
            csrs.push_back(it.csr_plain);
            if (it.srel == kEllipsis) {
              dfeed.push_back(it.csr_plain);
              dfeed_type.push_back({it.csr_plain, nd.type});
            }
          }
          if (it.srel != kEllipsis) next = it.target;
        } else if (it.kind == IT_COMPUTED) {
          next = it.target;
        } else if (it.kind == IT_ARROW) {
          if (ext_edges(it)) return false;
          if (it.target == kNoNode) continue;
          if (has_rows(it.csr_plain)) csrs.push_back(it.csr_plain);
          next = it.target;
        } else {
          return false;  // a nested join (IT_SUB)
        }
        if (next != kNone) {
          if (next >= nf) return false;
          if (!seen[next]) seen[next] = 1, stack.push_back(next);
        }
      }
    }
    return true;
  };
  std::vector<LabelPlan> plans;
  std::vector<uint32_t> csrs_all, hubs_all;
  for (uint32_t p = 0; p < nf && p < R && p < 0xFFFFu; ++p) {
    const DevNode& nd = nodes[p];
    LabelPlan pl;
    pl.p = p;
    if (hub[p]) {  // a hub root (group#member@user): its own vertex is the only V, no slot
      hubs_all.push_back(p);
      plans.push_back(std::move(pl));
      continue;
    }
    if (!sc.rels[p].is_perm) continue;
    if (nd.kind == NK_EXCLUDE || nd.kind == NK_INTERSECT) {
      if (nd.count > (uint32_t)kLjTerms) continue;
      for (uint32_t k = 0; k < nd.count; ++k) {
        pl.terms.push_back(items[nd.first + k].target);
        if (nd.kind == NK_EXCLUDE && k > 0) pl.neg |= (uint8_t)(1u << k);
      }
    } else if (nd.kind == NK_UNION || nd.kind == NK_RELATION) {
      pl.terms.push_back(p);
    } else {
      continue;
    }
    std::vector<uint32_t> cs, hs;
    bool ok = true;
    for (uint32_t t : pl.terms) ok = ok && t < nf && flattenable(t, cs, hs, pl.cav);
    if (!ok) continue;
    csrs_all.insert(csrs_all.end(), cs.begin(), cs.end());
    hubs_all.insert(hubs_all.end(), hs.begin(), hs.end());
    plans.push_back(std::move(pl));
  }
  if (plans.empty()) return;
  // nothing to gain where the closure join already answers every root the labels would (a
  // partitioned engine needs them: its checks go through the partitioned label join)
  if (!ds.cj_host.empty() && !e.part_set) {
    bool all_cj = true;
    for (const LabelPlan& pl : plans)
      all_cj &= pl.p * 2 + 1 < ds.cj_host.size() && reinterpret_cast<const uint16_t*>(ds.cj_host.data())[pl.p] != 0xFFFFu;
    if (all_cj) return;
  }
  // the hubs the roots reach, closed over the hubs' usersets
  // (hierarchy edges are read on the host; the subjects the hubs list directly stay on the device)
  std::vector<char> used(nf, 0);
  for (size_t k = 0; k < hubs_all.size(); ++k) {
    const uint32_t h = hubs_all[k];
    if (used[h]) continue;
    used[h] = 1;
    for (uint32_t n : loc[h])
      for (uint32_t j = 0; j < nodes[n].count; ++j) {
        const DevItem& it = items[nodes[n].first + j];
        if (it.srel == kEllipsis) continue;
        if (has_rows(it.csr_plain)) csrs_all.push_back(it.csr_plain);
        hubs_all.push_back(it.target);
      }
  }
  pc.mark("plans");
  // 3. host copies of every CSR the flattening and the hierarchy read
  std::sort(csrs_all.begin(), csrs_all.end());
  csrs_all.erase(std::unique(csrs_all.begin(), csrs_all.end()), csrs_all.end());
  // the tables depend on these CSRs (and the hubs' direct-subject ones), the roots' heights and the
  // object counts: a Watch batch that changed none of them keeps the previous snapshot's tables;
  // one that changed only direct grants (`dfeed`: the users listed in resource slots) keeps them
  // too, and marks the subjects it changed (lj_dirty_path)
  std::sort(dfeed.begin(), dfeed.end());
  dfeed.erase(std::unique(dfeed.begin(), dfeed.end()), dfeed.end());
  std::vector<uint64_t> key, dkey;
  std::vector<const uint32_t*> hkey;
  std::vector<uint32_t> hroots;
  {
    std::vector<uint32_t> all = csrs_all;
    for (uint32_t h = 0; h < nf; ++h)
      if (used[h])
        for (uint32_t n : loc[h])
          for (uint32_t j = 0; j < nodes[n].count; ++j) {
            const DevItem& it = items[nodes[n].first + j];
            if (nodes[n].kind == NK_RELATION && it.srel == kEllipsis && it.stype == U && has_rows(it.csr_plain))
              all.push_back(it.csr_plain);
          }
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    for (uint32_t c : all) {
      std::vector<uint64_t>& k = std::binary_search(dfeed.begin(), dfeed.end(), c) ? dkey : key;
      k.insert(k.end(), {c, (uint64_t)(uintptr_t)table[c].nbr, info[c].n_edges, table[c].n_rows});
    }
    for (const LabelPlan& pl : plans) {
      key.push_back(pl.p);
      hkey.push_back(pl.p < ds.hgt.size() ? ds.hgt[pl.p] : nullptr);
      hroots.push_back(pl.p);
    }
    for (const TypeInterner& ti : e.interner) key.push_back(ti.count);
    key.push_back(max_depth);
  }
  auto adopt_tables = [&](const DeviceSnapshot& old) {
    // (taken over at publish: the current snapshot keeps them, and its checks keep running, until
    // the new one replaces it — engine.hip device_publish)
    ds.adopt_h.insert(ds.adopt_h.end(), old.lj_ptrs.begin(), old.lj_ptrs.end());
    ds.lj_ptrs = old.lj_ptrs;
    ds.lj_host = old.lj_host;
    ds.lj_o_meta = old.lj_o_meta;
    ds.lj_sw = old.lj_sw;
    ds.lj_bits = old.lj_bits;
    ds.lj_preferred = old.lj_preferred;
    ds.lj_cav = old.lj_cav;
    ds.lj_dirty = old.lj_dirty;
    ds.lj_dirty_n = old.lj_dirty_n;
    ds.lj_users = old.lj_users;
    ds.lj_af = old.lj_af;
    ds.lj_afp = old.lj_afp;
    ds.lj_afp_n = old.lj_afp_n;
    ds.lj_anc = old.lj_anc;
    ds.lj_af_base = old.lj_af_base;
    ds.lj_af_rows = old.lj_af_rows;
    ds.lj_dtype = old.lj_dtype;
    ds.lj_dov = old.lj_dov;
    ds.lj_key = key;
    ds.lj_dkey = dkey;
    ds.lj_hgt = hkey;
    ds.lj_bytes = old.lj_bytes;
    ds.bytes += old.lj_bytes;
  };
  if (e.dev && !e.dev->lj_host.empty() && e.dev->lj_key == key && e.dev->lj_dkey == dkey && e.dev->lj_hgt == hkey) {
    adopt_tables(*e.dev);
    return;
  }
  // which roots read each direct-grant CSR on their resource's own object (through computed
  // usersets only), and which CSRs some root reads further away (through an arrow or a userset)
  std::map<uint32_t, std::vector<uint32_t>> own_roots;
  std::vector<uint32_t> own_only;
  {
    std::set<uint32_t> remote;
    for (const LabelPlan& pl : plans)
      for (uint32_t t : pl.terms) {
        std::vector<std::pair<uint32_t, bool>> st{{t, false}};
        std::vector<uint8_t> seen(nf, 0);
        seen[t] = 1;
        while (!st.empty()) {
          const auto [n, far] = st.back();
          st.pop_back();
          if (hub[n]) continue;
          const DevNode& nd = nodes[n];
          for (uint32_t k = 0; k < nd.count; ++k) {
            const DevItem& it = items[nd.first + k];
            uint32_t next = kNone;
            bool nfar = far;
            if (nd.kind == NK_RELATION && it.kind == IT_KIND) {
              if (it.srel == kEllipsis) {
                for (uint32_t c : {it.csr_plain, it.csr_ext})
                  if (has_rows(c)) {
                    if (far) remote.insert(c);
                    else own_roots[c].push_back(pl.p);
                  }
              } else {
                next = it.target, nfar = true;
              }
            } else if (nd.kind == NK_UNION && it.kind == IT_COMPUTED) {
              next = it.target;
            } else if (nd.kind == NK_UNION && it.kind == IT_ARROW && it.target != kNoNode) {
              next = it.target, nfar = true;
            }
            if (next < nf && !(seen[next] & (nfar ? 2 : 1))) {
              seen[next] |= nfar ? 2 : 1;
              st.push_back({next, nfar});
            }
          }
        }
      }
    for (auto& [c, v] : own_roots) {
      std::sort(v.begin(), v.end());
      v.erase(std::unique(v.begin(), v.end()), v.end());
      if (!remote.count(c)) own_only.push_back(c);
    }
  }
  const char* why = "";
  if (e.dev && !e.dev->lj_host.empty() && e.dev->lj_key == key &&
      lj_dirty_path(e, ds, dkey, hkey, max_depth, own_only, hroots, why)) {
    adopt_tables(*e.dev);
    lj_mark_dirty(e, ds, dkey, own_roots);
    pc.mark("dirty");
    return;
  }
  if (pc.on && e.dev && !e.dev->lj_host.empty())
    pc.line += std::string(" rebuild=\"") + (e.dev->lj_key == key ? why : "structure") + "\"";
  auto lalloc = [&](size_t bytes) {
    uint32_t* q = slot_alloc(ds, bytes);
    ds.lj_ptrs.push_back(q);
    ds.lj_bytes += bytes;
    return q;
  };
  std::unordered_map<uint32_t, HostRows> rows;
  for (uint32_t c : csrs_all) {
    HostRows& h = rows[c];
    h.n_rows = table[c].n_rows;
    h.off.resize((size_t)h.n_rows + 1);
    HIP_OK(hipMemcpy(h.off.data(), table[c].off, h.off.size() * 4, hipMemcpyDeviceToHost));
    h.nbr.resize(info[c].n_edges);
    if (!h.nbr.empty()) HIP_OK(hipMemcpy(h.nbr.data(), table[c].nbr, h.nbr.size() * 4, hipMemcpyDeviceToHost));
    if (table[c].is_ext && !h.nbr.empty()) {
      h.cav.resize(h.nbr.size());
      h.exp.resize(h.nbr.size());
      HIP_OK(hipMemcpy(h.cav.data(), table[c].cav, h.cav.size() * 4, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(h.exp.data(), table[c].exp_us, h.exp.size() * 8, hipMemcpyDeviceToHost));
    }
  }
  pc.mark("host_copies");
  // 4. the hierarchy: one vertex per object of every hub used, x -> y when x lists y#h'
  std::vector<uint64_t> base(nf, 0);
  uint64_t nv64 = 0;
  for (uint32_t h = 0; h < nf; ++h)
    if (used[h]) base[h] = nv64, nv64 += count_of(nodes[h].type);
  if (nv64 >= (1ull << 31)) return;
  const uint32_t NV = (uint32_t)nv64;
  std::vector<std::pair<uint32_t, uint32_t>> edges;    // (parent, child)
  std::vector<std::pair<uint32_t, uint64_t>> dsrc;     // (direct-subject CSR of a hub, its vertex base)
  for (uint32_t h = 0; h < nf; ++h) {
    if (!used[h]) continue;
    const uint32_t nh = count_of(nodes[h].type);
    for (uint32_t n : loc[h]) {
      if (nodes[n].kind != NK_RELATION) continue;
      for (uint32_t j = 0; j < nodes[n].count; ++j) {
        const DevItem& it = items[nodes[n].first + j];
        if (!has_rows(it.csr_plain)) continue;
        if (it.srel == kEllipsis) {
          if (it.stype == U) dsrc.push_back({it.csr_plain, base[h]});  // (other types never match a U check)
          continue;
        }
        const HostRows& hr = rows.at(it.csr_plain);
        const uint32_t nt = count_of(nodes[it.target].type);
        for (uint32_t x = 0; x < hr.n_rows && x < nh; ++x)
          for (uint32_t q = hr.off[x]; q < hr.off[x + 1]; ++q) {
            const uint32_t y = hr.nbr[q];
            if (y < nt) edges.push_back({(uint32_t)(base[h] + x), (uint32_t)(base[it.target] + y)});
          }
      }
    }
  }
  pc.mark("edges");
  std::vector<uint32_t> poff((size_t)NV + 1, 0), pnbr(edges.size()), coff((size_t)NV + 1, 0), cnbr(edges.size());
  for (auto& ed : edges) ++poff[ed.second + 1], ++coff[ed.first + 1];
  for (uint32_t v = 0; v < NV; ++v) poff[v + 1] += poff[v], coff[v + 1] += coff[v];
  {
    std::vector<uint32_t> pa(poff.begin(), poff.end() - 1), ca(coff.begin(), coff.end() - 1);
    for (auto& ed : edges) pnbr[pa[ed.second]++] = ed.first, cnbr[ca[ed.first]++] = ed.second;
  }
  edges.clear();
  edges.shrink_to_fit();
  std::vector<uint32_t> lab, cov_off, cov_pre;
  uint32_t n_cyclic = 0;
  hier_labels_any(NV, poff, pnbr, coff, cnbr, lab, cov_off, cov_pre, n_cyclic);
  // a hub root's vertices at or above the depth budget are deferred (the end word's top bit)
  bool any_hub_root = false;
  for (const LabelPlan& pl : plans) {
    if (!pl.terms.empty()) continue;
    any_hub_root = true;
    const uint32_t p = pl.p;
    if (p < ds.hgt.size() && ds.hgt[p] && ds.hcount[p]) {
      std::vector<uint32_t> hh(ds.hcount[p]);
      HIP_OK(hipMemcpy(hh.data(), ds.hgt[p], hh.size() * 4, hipMemcpyDeviceToHost));
      const uint32_t nh = count_of(nodes[p].type);
      for (uint32_t x = 0; x < nh; ++x)
        if (x >= hh.size() || hh[x] >= max_depth) lab[2 * (base[p] + x) + 1] |= kLjDeep;
    }
  }
  const uint32_t bits = NV < (1u << 24) - 1u ? 24u : 32u;
  const uint32_t n_users = count_of(U);
  const uint32_t n_users_loc = part_local_count(n_users, prank, P);  // (P = 1: n_users)
  // a hub that lists the wildcard holds every subject: not labelled
  {
    std::vector<void*> tmp;
    unsigned* flag = dalloc<unsigned>(tmp, 1);
    unsigned hw = 0;
    try {
      HIP_OK(hipMemset(flag, 0, 4));
      for (auto& [c, b] : dsrc)
        hipLaunchKernelGGL(k_any_wildcard, dim3(grid_for(info[c].n_edges)), dim3(kBlock), 0, 0, table[c].nbr,
                           (unsigned long long)info[c].n_edges, flag);
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemcpy(&hw, flag, 4, hipMemcpyDeviceToHost));
    } catch (...) {
      free_list(tmp);
      throw;
    }
    free_list(tmp);
    if (hw) return;
  }
  pc.mark("hierarchy");
  // 4b. the arrow forest (a dirty subject's checks, k_label_join round 2): the objects a
  // resource's flattening visits are those its arrows and non-hub usersets lead to; when every
  // object leads to at most one other (a document's folder, a folder's parent) they form a forest,
  // and the grants flattened into R's slot are those of R and its ancestors. Preorder intervals
  // over it let the join test "X is R or an ancestor of R" in one compare: a changed grant of the
  // subject on X touches R's slot only then. No forest (an object with two such edges, a cycle, a
  // partitioned graph): a dirty subject's checks defer, as before.
  std::vector<uint32_t> af_base(sc.types.size(), kNone), af_rows(sc.types.size(), 0), af_lab;
  std::vector<uint32_t> par, via;  // per forest vertex: its parent (kNone: a root), the CSR of that edge
  if (P == 1) {
    struct Trav {
      uint32_t csr;
      uint16_t src, dst;
    };
    std::vector<Trav> trav;
    std::vector<char> vtype(sc.types.size(), 0);
    for (const LabelPlan& pl : plans) {
      if (pl.terms.empty()) continue;
      vtype[nodes[pl.p].type] = 1;
      for (uint32_t t : pl.terms) {
        std::vector<uint32_t> st{t};
        std::vector<char> seen(nf, 0);
        seen[t] = 1;
        while (!st.empty()) {
          const uint32_t n = st.back();
          st.pop_back();
          if (hub[n]) continue;
          const DevNode& nd = nodes[n];
          for (uint32_t k = 0; k < nd.count; ++k) {
            const DevItem& it = items[nd.first + k];
            uint32_t next = kNone;
            if (nd.kind == NK_UNION && it.kind == IT_COMPUTED) next = it.target;
            else if ((nd.kind == NK_UNION && it.kind == IT_ARROW) || (nd.kind == NK_RELATION && it.kind == IT_KIND && it.srel != kEllipsis)) {
              if (it.target == kNoNode || it.target >= nf) continue;
              next = it.target;
              if (!hub[next] && has_rows(it.csr_plain)) trav.push_back({it.csr_plain, nd.type, nodes[next].type});
            }
            if (next < nf && !seen[next]) seen[next] = 1, st.push_back(next);
          }
        }
      }
    }
    for (const Trav& tv : trav) vtype[tv.src] = vtype[tv.dst] = 1;
    uint64_t nva = 0;
    for (size_t t = 0; t < vtype.size(); ++t)
      if (vtype[t]) af_base[t] = (uint32_t)nva, af_rows[t] = count_of((uint32_t)t), nva += af_rows[t];
    bool forest = nva > 0 && nva < (1ull << 31);
    if (forest) par.assign(nva, kNone), via.assign(nva, kNone);
    std::sort(trav.begin(), trav.end(), [](const Trav& a, const Trav& b) { return a.csr < b.csr; });
    trav.erase(std::unique(trav.begin(), trav.end(), [](const Trav& a, const Trav& b) { return a.csr == b.csr; }), trav.end());
    for (const Trav& tv : trav) {
      if (!forest) break;
      const HostRows& hr = rows.at(tv.csr);
      const uint32_t nx = std::min(hr.n_rows, af_rows[tv.src]), ny = af_rows[tv.dst];
      for (uint32_t x = 0; x < nx && forest; ++x)
        for (uint32_t q = hr.off[x]; q < hr.off[x + 1]; ++q) {
          const uint32_t y = hr.nbr[q];
          if (y == kWildcard || y >= ny) continue;
          const uint32_t v = af_base[tv.src] + x, p = af_base[tv.dst] + y;
          if (v == p || (par[v] != kNone && par[v] != p)) {
            forest = false;
            break;
          }
          par[v] = p;
          via[v] = tv.csr;
        }
    }
    if (forest) {  // preorder over the children, from every parentless vertex
      const uint32_t NVa = (uint32_t)nva;
      std::vector<uint32_t> coff2((size_t)NVa + 1, 0), cn2;
      for (uint32_t v = 0; v < NVa; ++v)
        if (par[v] != kNone) ++coff2[par[v] + 1];
      for (uint32_t v = 0; v < NVa; ++v) coff2[v + 1] += coff2[v];
      cn2.resize(coff2[NVa]);
      {
        std::vector<uint32_t> at(coff2.begin(), coff2.end() - 1);
        for (uint32_t v = 0; v < NVa; ++v)
          if (par[v] != kNone) cn2[at[par[v]]++] = v;
      }
      af_lab.assign(2 * (size_t)NVa, 0);
      uint32_t ctr = 0, done = 0;
      std::vector<std::pair<uint32_t, uint32_t>> stk;  // (vertex, next child)
      for (uint32_t r0 = 0; r0 < NVa; ++r0) {
        if (par[r0] != kNone) continue;
        stk.push_back({r0, coff2[r0]});
        af_lab[2 * (size_t)r0] = ctr++;
        while (!stk.empty()) {
          auto& [v, c] = stk.back();
          if (c < coff2[v + 1]) {
            const uint32_t ch = cn2[c++];
            af_lab[2 * (size_t)ch] = ctr++;
            stk.push_back({ch, coff2[ch]});
          } else {
            af_lab[2 * (size_t)v + 1] = ctr;
            ++done;
            stk.pop_back();
          }
        }
      }
      if (done != NVa) forest = false;  // (a cycle: vertices no root reaches)
    }
    if (!forest) {
      af_lab.clear();
      par.clear();
      via.clear();
      std::fill(af_base.begin(), af_base.end(), kNone);
    }
    if (pc.on) pc.line += std::string(" forest=") + (forest ? std::to_string(nva) : "none");
  }
  // 5. resource slots: flatten every term of every root over every resource
  std::vector<const uint32_t*> hgt_dev(plans.size(), nullptr);
  auto flatten = [&](uint32_t r, uint32_t t, Flat& f, std::vector<uint64_t>& stack, std::vector<uint64_t>& seen) {
    f.D.clear();
    f.V.clear();
    f.C.clear();
    f.wild = f.over = false;
    stack.assign(1, ((uint64_t)t << 32) | r);
    seen.clear();
    while (!stack.empty()) {
      const uint64_t s = stack.back();
      stack.pop_back();
      const uint32_t n = (uint32_t)(s >> 32), x = (uint32_t)s;
      if (hub[n]) {
        if (x < count_of(nodes[n].type)) f.V.push_back((uint32_t)(base[n] + x));
        if (f.V.size() > kLjFlatCap) return f.over = true, void();
        continue;
      }
      if (P > 1 && part_owner(x, P) != prank) return f.over = true, void();  // another rank's rows
      if (std::find(seen.begin(), seen.end(), s) != seen.end()) continue;
      seen.push_back(s);
      if (seen.size() > 256) return f.over = true, void();  // (a long arrow chain: the bundles walk it)
      const DevNode& nd = nodes[n];
      for (uint32_t k = 0; k < nd.count; ++k) {
        const DevItem& it = items[nd.first + k];
        if (nd.kind == NK_UNION && it.kind == IT_COMPUTED) {
          stack.push_back(((uint64_t)it.target << 32) | x);
          continue;
        }
        if (nd.kind == NK_RELATION && it.srel == kEllipsis && it.stype == U && has_rows(it.csr_ext)) {
          // caveated / expiring direct subjects: a caveat decided by the stored context alone is a
          // plain edge or none (Engine::caveat_static); a partial one a caveated pair; an expiring
          // relationship is for the bundles (its visibility depends on the check's time)
          const HostRows& hx = rows.at(it.csr_ext);
          if (x < hx.n_rows)
            for (uint32_t q = hx.off[x]; q < hx.off[x + 1]; ++q) {
              if (hx.exp[q] != 0) return f.over = true, void();
              const uint32_t y = hx.nbr[q], cv = hx.cav[q];
              const uint8_t st = cv < e.caveat_static.size() ? e.caveat_static[cv] : (uint8_t)cel::PARTIAL;
              if (st == cel::FALSE) continue;
              if (st == cel::TRUE) {
                if (y == kWildcard) f.wild = true;
                else f.D.push_back(y);
              } else {
                f.C.push_back(y == kWildcard ? kLjCavWild : y);
                f.C.push_back(cv);
              }
            }
          if (f.C.size() > 2 * kLjFlatCap) return f.over = true, void();
        }
        if (!has_rows(it.csr_plain) || (nd.kind == NK_UNION && (it.kind != IT_ARROW || it.target == kNoNode))) continue;
        const HostRows& hr = rows.at(it.csr_plain);
        if (x >= hr.n_rows) continue;
        for (uint32_t q = hr.off[x]; q < hr.off[x + 1]; ++q) {
          const uint32_t y = hr.nbr[q];
          if (nd.kind == NK_RELATION && it.srel == kEllipsis) {
            if (it.stype != U) break;
            if (y == kWildcard) f.wild = true;
            else f.D.push_back(y);
          } else if (y != kWildcard) {
            stack.push_back(((uint64_t)it.target << 32) | y);
          }
        }
        if (f.D.size() > kLjFlatCap || stack.size() > 16 * kLjFlatCap) return f.over = true, void();
      }
    }
    std::sort(f.D.begin(), f.D.end());
    f.D.erase(std::unique(f.D.begin(), f.D.end()), f.D.end());
    if (!f.C.empty()) {  // caveated pairs once each (kept beside a plain grant of the same user:
                         // the check still evaluates the caveat, which may fail)
      std::vector<std::pair<uint32_t, uint32_t>> cp;
      for (size_t q = 0; q < f.C.size(); q += 2) cp.push_back({f.C[q], f.C[q + 1]});
      std::sort(cp.begin(), cp.end());
      cp.erase(std::unique(cp.begin(), cp.end()), cp.end());
      f.C.clear();
      for (auto& [u, cv] : cp) f.C.push_back(u | kLjCav), f.C.push_back(cv);
    }
    // V as intervals, nested ones dropped (an interval inside another adds nothing)
    std::vector<std::pair<uint32_t, uint32_t>> iv;
    for (uint32_t v : f.V) iv.push_back({lab[2 * (size_t)v] & ~kSlotOverflow, lab[2 * (size_t)v + 1] & ~kLjDeep});
    std::sort(iv.begin(), iv.end(), [](auto& a, auto& b) { return a.first < b.first || (a.first == b.first && a.second > b.second); });
    f.V.clear();
    uint32_t reach = 0;
    bool any = false;
    for (auto& [lo, hi] : iv) {
      if (any && hi <= reach) continue;
      f.V.push_back(lo);
      f.V.push_back(hi - lo);
      reach = hi;
      any = true;
    }
  };
  // per root: its heights (a resource at or above the budget is deferred) and a sample of its
  // slot sizes (16 words when nearly every resource fits, else 32)
  std::vector<std::vector<uint32_t>> hgt_host(plans.size());
  for (size_t k = 0; k < plans.size(); ++k) {
    const uint32_t p = plans[k].p;
    if (plans[k].terms.empty()) continue;
    if (p < ds.hgt.size() && ds.hgt[p] && ds.hcount[p]) {
      hgt_host[k].resize(ds.hcount[p]);
      HIP_OK(hipMemcpy(hgt_host[k].data(), ds.hgt[p], (size_t)ds.hcount[p] * 4, hipMemcpyDeviceToHost));
    }
  }
  // inline slots of 24-bit fields (LjEnt24) when every entry fits: users (below the caveated-pair
  // flag when a root has caveated pairs), hierarchy preorder numbers and lengths, caveat instances
  bool any_cav = false;
  for (const LabelPlan& pl : plans) any_cav |= pl.cav;
  const bool can_pack = NV < 0xFFFFFFu && n_users < (any_cav ? 0x7FFFFFu : 0xFFFFFFu) &&
                        e.caveat_static.size() < 0xFFFFFFu;
  bool pack = false;
  auto words_in = [&](const std::vector<Flat>& fs, bool& inline_ok, bool p24) {
    uint32_t fields = 0;
    inline_ok = true;
    for (const Flat& f : fs) {
      fields += (uint32_t)(f.D.size() + f.C.size() + f.V.size());
      inline_ok &= f.D.size() + f.C.size() <= kLjMaxD && f.V.size() / 2 <= kLjMaxV;
    }
    return p24 ? (32u + 24u * fields + 31u) / 32u : 1u + fields;
  };
  auto words_of = [&](const std::vector<Flat>& fs, bool& inline_ok) { return words_in(fs, inline_ok, pack); };
  // the slot width and the encoding from a sample of every root's resources: 16 words when nearly
  // every resource fits, else 32; 24-bit fields only where they buy something — a narrower slot,
  // or clearly fewer extension records (their decoding costs ALU per entry: config 3, whose
  // records fit 16 words either way, ran 7 % slower packed)
  uint32_t sw32 = 16, sw24 = 16;
  uint64_t n_all = 0, ext32 = 0, ext24 = 0;
  for (LabelPlan& pl : plans) {
    if (pl.terms.empty()) continue;
    const uint32_t n_res = part_local_count(count_of(nodes[pl.p].type), prank, P);  // (this rank's)
    const uint32_t n_samp = std::min<uint32_t>(n_res, 4096);
    uint32_t fit32 = 0, fit24 = 0;
    std::vector<std::pair<uint32_t, uint32_t>> wds;  // (words unpacked, packed) of the inline ones
    std::vector<Flat> fs(pl.terms.size());
    std::vector<uint64_t> st, seen;
    for (uint32_t k = 0; k < n_samp; ++k) {
      const uint32_t r = (uint32_t)(((uint64_t)k * 2654435761ull) % std::max<uint32_t>(n_res, 1)) * P + prank;
      bool over = false;
      for (size_t t = 0; t < pl.terms.size(); ++t) flatten(r, pl.terms[t], fs[t], st, seen), over |= fs[t].over;
      if (over) continue;
      bool ok;
      const uint32_t w32 = words_in(fs, ok, false), w24 = words_in(fs, ok, true);
      if (!ok) {
        ++ext32, ++ext24, ++n_all;
        continue;
      }
      fit32 += w32 <= 16, fit24 += w24 <= 16;
      wds.push_back({w32, w24});
      ++n_all;
    }
    const uint32_t need32 = fit32 >= n_samp - n_samp / 32 ? 16u : 32u;
    const uint32_t need24 = fit24 >= n_samp - n_samp / 32 ? 16u : 32u;
    for (auto& [a, b] : wds) ext32 += a > need32, ext24 += b > need24;
    pl.sw_need = need32;
    sw32 = std::max(sw32, need32);
    sw24 = std::max(sw24, need24);
  }
  // packed when it removes extension records (config 2: 3 % -> 0.15 % of the resources), or
  // narrows the slot without adding them (config 3 at 16 words: 0.01 % -> 0.3 %, and a wave waits
  // for its slowest lane's extra round trip — 9.0 vs 9.9 G checks/s unpacked)
  pack = can_pack && ((ext24 + n_all / 50 < ext32) || (sw24 < sw32 && ext24 <= ext32 + n_all / 1000));
  if (const char* f = debug_env("GCK_DEBUG_LJ_PACK")) pack = can_pack && atoi(f) != 0;  // (an A/B of the encoding)
  uint32_t sw = pack ? sw24 : sw32;
  if (pc.on)
    pc.line += " sample[n=" + std::to_string(n_all) + " ext32=" + std::to_string(ext32) + " ext24=" + std::to_string(ext24) +
               " sw32=" + std::to_string(sw32) + " sw24=" + std::to_string(sw24) + "]";
  // memory: every root's slots plus the user slots must take at most half of the free HBM
  {
    uint64_t need = (uint64_t)n_users_loc * kUSlotWords * 4;
    for (const LabelPlan& pl : plans)
      if (!pl.terms.empty()) need += (uint64_t)part_local_count(count_of(nodes[pl.p].type), prank, P) * sw * 4;
    size_t free_b = 0, total_b = 0;
    HIP_OK(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b / 2) return;
  }
  pc.mark("sizing");
  // user slots over the hierarchy (closure.inc k_user_slots_1p: the covers of the vertices listing
  // each subject, inline or as a list)
  const uint32_t* uslot = nullptr;
  const uint32_t* ulist = nullptr;
  const uint32_t* lab_dev = nullptr;
  {
    std::vector<void*> tmp;
    try {
      // (kept with the snapshot when a hub root reads its vertex's interval from it)
      // (+64 B: k_label_join loads kLines - 1 lines from a hub root's label line, and the second
      // one of the array's last line would lie past the end)
      uint32_t* d_lab = any_hub_root ? lalloc(std::max<size_t>(lab.size(), 1) * 4 + 64)
                                     : dalloc<uint32_t>(tmp, std::max<size_t>(lab.size(), 1));
      if (any_hub_root) HIP_OK(hipMemset(d_lab + lab.size(), 0, 64));
      lab_dev = d_lab;
      uint32_t* d_coff = dalloc<uint32_t>(tmp, cov_off.size());
      uint32_t* d_cpre = dalloc<uint32_t>(tmp, std::max<size_t>(cov_pre.size(), 1));
      // subject -> the vertices listing it, a CSR over the subject type built on the device from
      // every hub's direct-subject CSRs: counts, scan, scatter with each hub's vertex base
      uint64_t n_pairs = 0;
      for (auto& [c, b] : dsrc) n_pairs += info[c].n_edges;
      if (n_pairs >= (1ull << 32)) throw Error(GCK_E_CAPACITY, "label join: too many direct memberships");
      const uint32_t nu = n_users_loc;  // the subjects whose slots this rank holds
      uint32_t* d_doff = dalloc<uint32_t>(tmp, (size_t)nu + 1);
      uint32_t* d_dnbr = dalloc<uint32_t>(tmp, std::max<uint64_t>(n_pairs, 1));
      uint32_t* d_cnt = dalloc<uint32_t>(tmp, std::max<uint32_t>(nu, 1));
      HIP_OK(hipStreamSynchronize(nullptr));
      if (!lab.empty()) HIP_OK(hipMemcpy(d_lab, lab.data(), lab.size() * 4, hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy(d_coff, cov_off.data(), cov_off.size() * 4, hipMemcpyHostToDevice));
      if (!cov_pre.empty()) HIP_OK(hipMemcpy(d_cpre, cov_pre.data(), cov_pre.size() * 4, hipMemcpyHostToDevice));
      // (a partitioned graph: the subjects this rank owns, at their part_local index)
      HIP_OK(hipMemset(d_cnt, 0, (size_t)std::max<uint32_t>(nu, 1) * 4));
      for (auto& [c, b] : dsrc)
        hipLaunchKernelGGL(k_count_subjects_part, dim3(grid_for(info[c].n_edges)), dim3(kBlock), 0, 0, table[c].nbr,
                           (unsigned long long)info[c].n_edges, n_users, prank, P, d_cnt);
      HIP_OK(hipGetLastError());
      device_excl_scan(d_cnt, nu, d_doff);
      HIP_OK(hipMemcpy(d_cnt, d_doff, (size_t)std::max<uint32_t>(nu, 1) * 4, hipMemcpyDeviceToDevice));
      for (auto& [c, b] : dsrc)
        hipLaunchKernelGGL(k_transpose_scatter_base, dim3(grid_for(info[c].n_edges)), dim3(kBlock), 0, 0, table[c].off,
                           table[c].nbr, table[c].n_rows, (unsigned long long)info[c].n_edges, n_users, d_cnt, d_dnbr,
                           (uint32_t)b, prank, P);
      HIP_OK(hipGetLastError());
      uint32_t* s = lalloc((size_t)std::max<uint32_t>(nu, 1) * kUSlotWords * 4);
      uint32_t* list = nullptr;
      // (bidir.inc build_user_slots; the sizing above has already bounded the slots, and the lists
      // are allocated whatever is free)
      if (nu) list = build_user_slots(bits, d_doff, d_dnbr, nu, d_lab, d_coff, d_cpre, NV, s, lalloc).list;
      uslot = s;
      ulist = list;
    } catch (...) {
      free_list(tmp);
      throw;
    }
    free_list(tmp);
  }
  pc.mark("user_slots");
  const uint32_t* af_dev = nullptr;
  unsigned long long* afp_dev = nullptr;
  uint32_t* anc_dev = nullptr;
  if (!af_lab.empty()) {
    uint32_t* q = lalloc(af_lab.size() * 4);
    HIP_OK(hipMemcpy(q, af_lab.data(), af_lab.size() * 4, hipMemcpyHostToDevice));
    af_dev = q;
    // the parent edges for the chain walk (tupleset CSR << 32 | parent), with the forest
    std::vector<unsigned long long> afp(par.size());
    for (size_t v = 0; v < par.size(); ++v) afp[v] = ((unsigned long long)via[v] << 32) | par[v];
    afp_dev = reinterpret_cast<unsigned long long*>(lalloc(std::max<size_t>(afp.size(), 1) * 8));
    if (!afp.empty()) HIP_OK(hipMemcpy(afp_dev, afp.data(), afp.size() * 8, hipMemcpyHostToDevice));
    // each vertex's ancestors in one line (lj_chain_wave): its whole chain in one round
    std::vector<uint32_t> anc(par.size() * kAncWords, 0u);
    host_parallel(par.size(), 1 << 14, [&](size_t lo, size_t hi) {
      for (size_t v = lo; v < hi; ++v) {
        uint32_t* L = &anc[v * kAncWords];
        uint32_t n = 0, x = (uint32_t)v;
        while (par[x] != kNone) {
          if (n + 1 == kAncWords) {
            n |= kAncOver;
            break;
          }
          x = par[x];
          L[++n] = x;
        }
        L[0] = n;
      }
    });
    anc_dev = lalloc(std::max<size_t>(anc.size(), 1) * 4);
    if (!anc.empty()) HIP_OK(hipMemcpy(anc_dev, anc.data(), anc.size() * 4, hipMemcpyHostToDevice));
  }
  // 5b. chain programs (LjChain, lj_chain_walk): per term the sets of schema nodes its flattening
  // holds at each depth of the resource's forest chain — the nodes reached through computed
  // usersets on one object, then through the level's arrow on the parent — and the direct-user
  // classes those nodes read. Exact only where the walk can follow the flattening: every arrow of
  // a level over one tupleset CSR (the forest edge the walk checks), no userset to a node that is
  // not a hub (its objects would be other chains), unions and stored relations only. Otherwise the
  // root has no program and its overlay hits defer, as before.
  auto lj_chain_of = [&](const LabelPlan& pl, LjChain& ch) -> bool {
    std::memset(&ch, 0, sizeof(ch));
    std::memset(ch.first, kLjChainEnd, sizeof(ch.first));
    std::vector<std::vector<uint32_t>> sets;
    auto closure = [&](std::vector<uint32_t> st) {
      std::vector<char> seen(nf, 0);
      std::vector<uint32_t> out;
      while (!st.empty()) {
        const uint32_t n = st.back();
        st.pop_back();
        if (n >= nf || seen[n] || hub[n]) continue;
        seen[n] = 1;
        out.push_back(n);
        const DevNode& nd = nodes[n];
        if (nd.kind != NK_UNION) continue;
        for (uint32_t k = 0; k < nd.count; ++k)
          if (items[nd.first + k].kind == IT_COMPUTED) st.push_back(items[nd.first + k].target);
      }
      std::sort(out.begin(), out.end());
      return out;
    };
    for (size_t t = 0; t < pl.terms.size(); ++t) {
      std::vector<uint32_t> N = closure({pl.terms[t]});
      uint8_t* link = &ch.first[t];
      for (;;) {
        const auto f = std::find(sets.begin(), sets.end(), N);
        if (f != sets.end()) {
          *link = (uint8_t)(f - sets.begin());
          break;
        }
        if (sets.size() == kLjChainLvls) return false;
        LjChainLvl L{};
        L.arrow = 0xFFFFu;
        L.next = kLjChainEnd;
        uint32_t type = kNone, arrow = kNone;
        std::vector<uint32_t> targets;
        for (uint32_t n : N) {
          const DevNode& nd = nodes[n];
          if (type != kNone && nd.type != type) return false;
          type = nd.type;
          if (nd.kind == NK_NIL) continue;
          if (nd.kind != NK_RELATION && nd.kind != NK_UNION) return false;
          for (uint32_t k = 0; k < nd.count; ++k) {
            const DevItem& it = items[nd.first + k];
            if (nd.kind == NK_RELATION) {
              if (it.kind != IT_KIND) return false;
              if (it.srel != kEllipsis) {
                if (it.target == kNoNode || it.target >= nf || !hub[it.target]) return false;
                continue;  // (a hub's members: the slot's intervals)
              }
              if (it.stype != U) continue;
              for (uint32_t c : {it.csr_plain, it.csr_ext})
                if (has_rows(c)) {
                  if (L.n == kLjChainCls || c >= 0xFFFFu) return false;
                  L.csr[L.n++] = (uint16_t)c;
                }
            } else if (it.kind == IT_ARROW) {
              if (it.target == kNoNode || it.target >= nf || hub[it.target] || !has_rows(it.csr_plain)) continue;
              if (arrow != kNone && arrow != it.csr_plain) return false;
              arrow = it.csr_plain;
              targets.push_back(it.target);
            } else if (it.kind != IT_COMPUTED) {
              return false;
            }
          }
        }
        if (type == kNone || type >= af_base.size() || af_base[type] == kNone || (arrow != kNone && arrow >= 0xFFFFu)) return false;
        L.af_base = af_base[type];
        const size_t idx = sets.size();
        sets.push_back(N);
        ch.lvl[idx] = L;
        *link = (uint8_t)idx;
        if (targets.empty()) break;
        ch.lvl[idx].arrow = (uint16_t)arrow;
        link = &ch.lvl[idx].next;
        N = closure(targets);
      }
    }
    for (size_t t = 0; t < pl.terms.size(); ++t)
      if (ch.first[t] >= sets.size()) return false;
    for (size_t l = 0; l < sets.size(); ++l)
      if (ch.lvl[l].next != kLjChainEnd && ch.lvl[l].next >= sets.size()) return false;
    return true;
  };
  // resource slots, every root, in parallel over the resources; records that do not fit inline go
  // to the extension array (one per root)
  std::vector<LjMeta> metas;
  std::vector<uint16_t> root(nf, 0xFFFFu);
  for (size_t k = 0; k < plans.size(); ++k) {
    const LabelPlan& pl = plans[k];
    const uint32_t n_res = count_of(nodes[pl.p].type);
    if (pl.terms.empty()) {  // hub root: the "slot" is the vertex's interval in the labels
      LjMeta M{};
      M.uslot = uslot;
      M.ulist = ulist;
      M.rslot = lab_dev + 2 * base[pl.p];
      M.u_rows = n_users;
      M.r_rows = n_res;
      M.rtype = nodes[pl.p].type;
      M.utype = (uint16_t)U;
      M.n_terms = 0;
      root[pl.p] = (uint16_t)metas.size();
      metas.push_back(M);
      continue;
    }
    // (a partitioned graph: the resources this rank owns, slot li = resource li * P + rank)
    const uint32_t n_loc = part_local_count(n_res, prank, P);
    std::vector<uint32_t> slots((size_t)std::max<uint32_t>(n_loc, 1) * sw, 0);
    std::mutex ext_mu;
    std::vector<std::pair<uint32_t, std::vector<uint32_t>>> exts;  // (first slot of the chunk, records)
    std::atomic<uint64_t> n_ext{0}, n_over{0}, n_pairs{0};  // (GCK_DEBUG_PHASES: the slot formats)
    const std::vector<uint32_t>& hh = hgt_host[k];
    host_parallel(n_loc, 4096, [&](size_t lo, size_t hi) {
      std::vector<Flat> fs(pl.terms.size());
      std::vector<uint64_t> st, seen;
      std::vector<uint32_t> ext;
      for (size_t li = lo; li < hi; ++li) {
        const size_t r = li * P + prank;
        uint32_t* w = &slots[li * sw];
        if (!hh.empty() && (r >= hh.size() || hh[r] >= max_depth)) {
          w[0] = kLjHdrOverflow;
          continue;
        }
        bool over = false;
        for (size_t t = 0; t < pl.terms.size(); ++t) {
          flatten((uint32_t)r, pl.terms[t], fs[t], st, seen);
          over |= fs[t].over;
        }
        if (over) {
          w[0] = kLjHdrOverflow;
          ++n_over;
          continue;
        }
        for (const Flat& f : fs) n_pairs += f.C.size() / 2;
        bool ok;
        const uint32_t words = words_of(fs, ok);
        if (ok && words <= sw) {
          uint32_t hdr = 0, pos = 1, fld = 0;
          // a 24-bit field at bit 32 + 24 j of the slot (the caveated-pair flag and wildcard
          // re-encoded: LjEnt24)
          auto put24 = [&](uint32_t v) {
            const uint32_t b = 32u + 24u * fld++, i = b >> 5, sh = b & 31u;
            w[i] |= v << sh;
            if (sh > 8u) w[i + 1] |= v >> (32u - sh);
          };
          for (size_t t = 0; t < fs.size(); ++t) {
            const uint32_t nD = (uint32_t)(fs[t].D.size() + fs[t].C.size());
            hdr |= (nD | (uint32_t)(fs[t].V.size() / 2) << 5 | (fs[t].wild ? 1u : 0u) << 9) << (10 * t);
            if (pack) {
              for (uint32_t v : fs[t].D) put24(v);
              for (size_t q = 0; q < fs[t].C.size(); q += 2) {
                const uint32_t a = fs[t].C[q];
                put24(a == (kLjCav | kLjCavWild) ? 0xFFFFFFu : ((a & ~kLjCav) | LjEnt24::kCav));
                put24(fs[t].C[q + 1]);
              }
              for (uint32_t v : fs[t].V) put24(v);
            } else {
              for (uint32_t v : fs[t].D) w[pos++] = v;
              for (uint32_t v : fs[t].C) w[pos++] = v;
              for (uint32_t v : fs[t].V) w[pos++] = v;
            }
          }
          w[0] = hdr;
        } else {
          ++n_ext;
          w[0] = kLjHdrExt;
          w[1] = (uint32_t)ext.size();  // chunk-local; made global below
          uint32_t h0 = (uint32_t)fs.size();
          for (size_t t = 0; t < fs.size(); ++t) h0 |= (fs[t].wild ? 1u : 0u) << (8 + t);
          ext.push_back(h0);
          for (const Flat& f : fs) ext.push_back((uint32_t)(f.D.size() + f.C.size())), ext.push_back((uint32_t)(f.V.size() / 2));
          for (const Flat& f : fs) {
            ext.insert(ext.end(), f.D.begin(), f.D.end());
            ext.insert(ext.end(), f.C.begin(), f.C.end());
            ext.insert(ext.end(), f.V.begin(), f.V.end());
          }
        }
      }
      std::lock_guard<std::mutex> lk(ext_mu);
      exts.push_back({(uint32_t)lo, std::move(ext)});
    });
    if (pc.on)
      pc.line += " root" + std::to_string(pl.p) + "[n=" + std::to_string(n_loc) + " need=" + std::to_string(pl.sw_need) +
                 " ext=" + std::to_string(n_ext.load()) +
                 " deferred=" + std::to_string(n_over.load()) + " pairs=" + std::to_string(n_pairs.load()) + "]";
    std::sort(exts.begin(), exts.end(), [](auto& a, auto& b) { return a.first < b.first; });
    std::vector<uint32_t> ext_all;
    for (size_t c = 0; c < exts.size(); ++c) {
      const uint32_t lo = exts[c].first, hi = c + 1 < exts.size() ? exts[c + 1].first : n_loc;
      const uint32_t b = (uint32_t)ext_all.size();
      if (ext_all.size() + exts[c].second.size() >= (1ull << 31)) return;
      for (uint32_t r = lo; r < hi; ++r)
        if (slots[(size_t)r * sw] == kLjHdrExt) slots[(size_t)r * sw + 1] += b;
      ext_all.insert(ext_all.end(), exts[c].second.begin(), exts[c].second.end());
    }
    uint32_t* d_slots = lalloc(slots.size() * 4);
    HIP_OK(hipMemcpy(d_slots, slots.data(), slots.size() * 4, hipMemcpyHostToDevice));
    uint32_t* d_ext = nullptr;
    if (!ext_all.empty()) {
      d_ext = lalloc(ext_all.size() * 4);
      HIP_OK(hipMemcpy(d_ext, ext_all.data(), ext_all.size() * 4, hipMemcpyHostToDevice));
    }
    LjMeta M{};
    M.uslot = uslot;
    M.ulist = ulist;
    M.rslot = d_slots;
    M.rext = d_ext;
    M.u_rows = n_users;
    M.r_rows = n_res;
    M.rtype = nodes[pl.p].type;
    M.utype = (uint16_t)U;
    M.n_terms = (uint8_t)pl.terms.size();
    M.neg = pl.neg;
    M.cav = pl.cav ? 1 : 0;
    M.pack = pack ? 1 : 0;
    M.apre = af_dev && af_base[M.rtype] != kNone ? af_dev + 2 * (size_t)af_base[M.rtype] : nullptr;
    M.chain = nullptr;
    if (M.apre && afp_dev) {
      LjChain ch;
      if (lj_chain_of(pl, ch)) {
        LjChain* q = reinterpret_cast<LjChain*>(lalloc(sizeof(LjChain)));
        HIP_OK(hipMemcpy(q, &ch, sizeof(LjChain), hipMemcpyHostToDevice));
        M.chain = q;
      }
      if (pc.on) {
        pc.line += std::string(" chain") + std::to_string(pl.p) + "=";
        if (!M.chain) pc.line += "no";
        for (size_t t = 0; M.chain && t < pl.terms.size(); ++t) pc.line += "t" + std::to_string(ch.first[t]);
        for (uint32_t l = 0; M.chain && l < kLjChainLvls && (ch.lvl[l].n || ch.lvl[l].arrow); ++l)
          pc.line += "[" + std::to_string(ch.lvl[l].af_base) + "," + std::to_string(ch.lvl[l].n) + "," +
                     std::to_string(ch.lvl[l].arrow) + "," + std::to_string(ch.lvl[l].next) + "]";
      }
    }
    root[pl.p] = (uint16_t)metas.size();
    metas.push_back(M);
  }
  std::vector<unsigned char> blob;
  auto put = [&](const void* src, size_t bytes) {
    const size_t o = (blob.size() + 15) & ~(size_t)15;
    blob.resize(o + bytes);
    std::memcpy(blob.data() + o, src, bytes);
    return (uint32_t)o;
  };
  pc.mark("res_slots");
  put(root.data(), root.size() * 2);
  const uint32_t o_meta = put(metas.data(), metas.size() * sizeof(LjMeta));
  if (blob.size() > kLjLdsBytes) return;  // (the slots stay allocated with the snapshot)
  // the closure join keeps the stage when it answers every root the labels answer (config 4's
  // tuned path); the labels take it when they cover every closure-join root and more
  bool covers = true, more = false;
  for (uint32_t p = 0; p < nf; ++p) {
    const bool in_cj = !ds.cj_host.empty() && p * 2 + 1 < ds.cj_host.size() &&
                       reinterpret_cast<const uint16_t*>(ds.cj_host.data())[p] != 0xFFFFu;
    const bool in_lj = root[p] != 0xFFFFu;
    covers &= !in_cj || in_lj;
    more |= in_lj && !in_cj;
  }
  ds.lj_preferred = covers && more;
  ds.lj_dkey = std::move(dkey);
  ds.lj_hgt = std::move(hkey);
  ds.lj_users = n_users;
  ds.lj_af = const_cast<uint32_t*>(af_dev);
  ds.lj_afp = afp_dev;
  ds.lj_afp_n = afp_dev ? (uint32_t)par.size() : 0u;
  ds.lj_anc = anc_dev;
  ds.lj_af_base = std::move(af_base);
  ds.lj_af_rows = std::move(af_rows);
  std::sort(dfeed_type.begin(), dfeed_type.end());
  dfeed_type.erase(std::unique(dfeed_type.begin(), dfeed_type.end()), dfeed_type.end());
  ds.lj_dtype = std::move(dfeed_type);
  ds.lj_dov = nullptr;  // (a fresh set of dirty subjects: the tables are new)
  for (const LabelPlan& pl : plans) ds.lj_cav |= pl.cav;
  ds.lj_key = std::move(key);
  ds.lj_host = std::move(blob);
  ds.lj_o_meta = o_meta;
  ds.lj_sw = sw;
  if (pc.on) pc.line += " sw=" + std::to_string(sw) + " bits=" + std::to_string(bits) + " pack=" + (pack ? "24" : "32");
  ds.lj_bits = bits;
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
      n_cont = ((w0 & ~(kSlotList | kSlotOverflow)) + 15u) / 16u;
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
    const uint32_t ng = v[0].x & ~(kSlotList | kSlotOverflow);
    const uint32_t* list = M.ulist + v[0].y;
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
      has = LjRecCovers{cont, uw[0] & ~(kSlotList | kSlotOverflow)}.any_in(lo, len);
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
      const LjRecCovers cr{cont, uw[0] & ~(kSlotList | kSlotOverflow)};
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
