// slot_pack.hpp — the 64-B user slot of the closure join's fast path (closure.inc): its layout, and
// the packing of an over-full user's cover entries. Plain C++ that host code compiles as well as
// the device (the slot-build kernels in closure.inc call it; gck_api.cpp exports it for the tests).
//
// Word 0 is the header, words 1-15 hold slot_cap<BITS>() cover entries of BITS bits each, packed
// from bit 32 (20 at 24 bits, 15 at 32). Three kinds of slot:
//
//   inline   header = the entry count; unused entries are all ones (above every interval).
//   overflow header = kSlotOverflow: the task rounds decide.
//   listed   header = kSlotList | kSlotLoOpen? | kSlotHiOpen? | count: the user's covers are `count`
//            entries of the list array at the offset in word 15 — sorted and without duplicates
//            when their raw number was at most kSlotSortMax. The entry positions before the last
//            two hold slot_inline_cap<BITS>() of those entries; the last two positions are the
//            offset's (word 15) and read as unused entries. What is left out is ONE run of
//            consecutive entries of the sorted list, the run whose open range (lo, hi) between its
//            inline neighbours is narrowest; the inline entries are stored rotated, the ones after
//            the run first, so that hi is entry 0 and lo the last inline entry. kSlotHiOpen: the
//            run ends the list (hi is the maximum); kSlotLoOpen: it begins the list (lo is below 0).
//            A check is HAS when an inline entry lies in one of the resource's intervals, NO when
//            none does and no interval [p, e) has p < hi and e > lo + 1 (it cannot hold a point of
//            (lo, hi), where every omitted entry lies), and goes to the list round otherwise.
//            A listed slot with both ends open and every inline entry unused (raw number above
//            kSlotSortMax) decides nothing itself.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GCK_SLOT_HD __host__ __device__
#else
#define GCK_SLOT_HD
#endif

namespace gck {

constexpr uint32_t kUSlotWords = 16;   // 64 B per user: header, cover entries
constexpr uint32_t kSlotOverflow = 0x80000000u;
constexpr uint32_t kSlotList = 0x40000000u;    // user slot: the covers are a list (word 15 = its offset in ucov)
constexpr uint32_t kSlotLoOpen = 0x20000000u;  // listed: the omitted run begins the sorted list
constexpr uint32_t kSlotHiOpen = 0x10000000u;  // listed: the omitted run ends it
constexpr uint32_t kSlotCount = 0x0FFFFFFFu;   // listed: the list's length
constexpr uint32_t kSlotSortMax = 64;          // raw entries of a user that are sorted and deduplicated (more: a plain list)
template <int BITS> constexpr int slot_cap() { return BITS == 24 ? 20 : 15; }
template <int BITS> constexpr int slot_inline_cap() { return slot_cap<BITS>() - 2; }  // of a listed slot
template <int BITS> constexpr uint32_t kSlotUnused = BITS == 32 ? 0xFFFFFFFFu : (1u << BITS) - 1u;

// every reader of a listed slot's list goes through these two
GCK_SLOT_HD inline uint32_t slot_list_count(uint32_t w0) { return w0 & kSlotCount; }
GCK_SLOT_HD inline uint32_t slot_list_off(const uint32_t* w) { return w[kUSlotWords - 1]; }

// Entry k of slot w (already zeroed there) := x; any k below slot_cap. (The inline slots of the
// full build are packed in registers instead: closure.inc slot_put_at.)
GCK_SLOT_HD inline void slot_put_dyn(uint32_t* w, uint32_t bits, uint32_t k, uint32_t x) {
  if (bits == 32) {
    w[1 + k] = x;
    return;
  }
  const uint32_t off = 32 + k * 24, wi = off / 32, sh = off % 32;
  w[wi] |= x << sh;
  if (sh + 24 > 32) w[wi + 1] |= x >> (32 - sh);
}

// e[0, n) sorted in place without its duplicates; returns how many are left. n is small
// (<= kSlotSortMax) and mostly sorted runs (each group's cover is ascending): insertion sort.
GCK_SLOT_HD inline uint32_t slot_sort_unique(uint32_t* e, uint32_t n) {
  for (uint32_t i = 1; i < n; ++i) {
    const uint32_t x = e[i];
    uint32_t j = i;
    for (; j > 0 && e[j - 1] > x; --j) e[j] = e[j - 1];
    e[j] = x;
  }
  uint32_t m = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (m == 0 || e[m - 1] != e[i]) e[m++] = e[i];
  return m;
}

// Where the omitted run of a listed slot begins: e[0, m) sorted and unique, n_in < m of them stay
// inline, e[s, s + m - n_in) are left out. The run's range is open: (e[s - 1], e[s + m - n_in]),
// with -1 and 2^32 - 1 beyond the list's ends; its width hi - (lo + 1) is the narrowest there is
// (the first such s).
GCK_SLOT_HD inline uint32_t slot_window(const uint32_t* e, uint32_t m, uint32_t n_in) {
  const uint32_t n_om = m - n_in;
  uint32_t best = 0, best_w = 0xFFFFFFFFu;
  for (uint32_t s = 0; s <= n_in; ++s) {
    const uint32_t lo1 = s ? e[s - 1] + 1u : 0u;
    const uint32_t hi = s + n_om < m ? e[s + n_om] : 0xFFFFFFFFu;
    if (hi - lo1 < best_w) best_w = hi - lo1, best = s;
  }
  return best;
}

// The slot of a user whose sorted, unique cover entries are e[0, m), its list at list_at: inline
// when they fit, listed with its window otherwise. bits: 24 or 32.
GCK_SLOT_HD inline void slot_pack_sorted(uint32_t bits, const uint32_t* e, uint32_t m, uint32_t list_at, uint32_t* w) {
  const uint32_t cap = bits == 24 ? (uint32_t)slot_cap<24>() : (uint32_t)slot_cap<32>();
  const uint32_t unused = bits == 24 ? kSlotUnused<24> : kSlotUnused<32>;
  for (uint32_t k = 0; k < kUSlotWords; ++k) w[k] = 0u;
  if (m <= cap) {
    for (uint32_t k = 0; k < cap; ++k) slot_put_dyn(w, bits, k, k < m ? e[k] : unused);
    w[0] = m;
    return;
  }
  const uint32_t n_in = cap - 2u, n_om = m - n_in, s = slot_window(e, m, n_in);
  uint32_t k = 0;
  for (uint32_t i = s + n_om; i < m; ++i) slot_put_dyn(w, bits, k++, e[i]);  // after the run: entry 0 = hi
  for (uint32_t i = 0; i < s; ++i) slot_put_dyn(w, bits, k++, e[i]);         // before it: the last = lo
  w[0] = kSlotList | (s == 0u ? kSlotLoOpen : 0u) | (s == n_in ? kSlotHiOpen : 0u) | m;
  w[kUSlotWords - 1] = list_at;
}

// A listed slot that decides nothing itself (the list's entries are neither sorted nor unique).
GCK_SLOT_HD inline void slot_pack_plain_list(uint32_t bits, uint32_t count, uint32_t list_at, uint32_t* w) {
  const uint32_t cap = bits == 24 ? (uint32_t)slot_cap<24>() : (uint32_t)slot_cap<32>();
  const uint32_t unused = bits == 24 ? kSlotUnused<24> : kSlotUnused<32>;
  for (uint32_t k = 0; k < kUSlotWords; ++k) w[k] = 0u;
  for (uint32_t k = 0; k < cap - 2u; ++k) slot_put_dyn(w, bits, k, unused);
  w[0] = kSlotList | kSlotLoOpen | kSlotHiOpen | count;
  w[kUSlotWords - 1] = list_at;
}

// ---- the 16-B front of a resource slot (24-bit snapshots) ----------------------------------------
// A resource slot (closure.inc kDSlotWords: word 0 the interval count or kSlotOverflow, word 1 zero,
// words 2 + 2k, 3 + 2k interval k as [start, end)) is read at random once per check; four fronts
// share the 64-B line that one slot fills, so more of them stay in the Infinity Cache between two
// uses. A front holds what the first half of a slot holds, in 128 bits:
//   word k (k < 3)  bits 0-23 start of interval k, bits 24-31 the low 8 bits of its length
//   word 3          bits 10k .. 10k+9 the high 10 bits of the length of interval k; bits 30-31 the count
// Lengths are kFrontLenBits (18) bits, starts 24, counts 0-3; unused intervals are zero. A resource
// whose slot does not fit — more than 3 intervals, an overflow slot, a nonzero word 1, a start of
// 2^24 or more, a length of 0 or above 2^18 - 1 (an end below its start wraps to one) — has the
// all-ones front kFrontReadSlot instead (the "read the slot" flag: in band, 2 + 3 x 42 bits leave
// none over), and so has a slot whose packed form would be all ones. The join then decides the
// check from its 64-B slot exactly as without fronts.
constexpr uint32_t kFrontWords = 4;
constexpr uint32_t kFrontV = 3;         // intervals of a front (= closure.inc kSlotHalfV)
constexpr uint32_t kFrontLenBits = 18;  // + 24 bits of start = 42 per interval
constexpr uint32_t kFrontLenMax = (1u << kFrontLenBits) - 1u;
constexpr uint32_t kFrontReadSlot = 0xFFFFFFFFu;  // every word of a flagged front

GCK_SLOT_HD inline bool front_flagged(const uint32_t* f) { return (f[0] & f[1] & f[2] & f[3]) == kFrontReadSlot; }

// The front of the slot d (16 words); returns whether it packed (false: flagged).
GCK_SLOT_HD inline bool front_pack(const uint32_t* d, uint32_t* f) {
  bool ok = !(d[0] & kSlotOverflow) && d[0] <= kFrontV && d[1] == 0u;
  for (uint32_t k = 0; k < kFrontWords; ++k) f[k] = 0u;
  for (uint32_t k = 0; k < kFrontV && ok; ++k) {
    const uint32_t lo = d[2 + 2 * k], len = d[3 + 2 * k] - lo;
    if (k >= d[0]) {
      ok = lo == 0u && d[3 + 2 * k] == 0u;  // (an unused interval is empty in the slot too)
      continue;
    }
    if (lo >> 24 || len == 0u || len > kFrontLenMax) {
      ok = false;
      continue;
    }
    f[k] = lo | (len & 255u) << 24;
    f[3] |= (len >> 8) << (10u * k);
  }
  for (uint32_t k = 2 + 2 * kFrontV; k < 16u && ok; ++k) ok = d[k] == 0u;  // (the slot's second half: empty)
  if (ok) f[3] |= d[0] << 30;
  if (!ok || front_flagged(f))
    for (uint32_t k = 0; k < kFrontWords; ++k) f[k] = kFrontReadSlot;
  return !front_flagged(f);
}

// Words 0-7 of the slot a packed (not flagged) front stands for; the slot's words 8-15 are zero.
GCK_SLOT_HD inline void front_unpack(const uint32_t* f, uint32_t* d) {
  d[0] = f[3] >> 30;
  d[1] = 0u;
  for (uint32_t k = 0; k < kFrontV; ++k) {
    const uint32_t lo = f[k] & 0xFFFFFFu, len = f[k] >> 24 | (f[3] >> (10u * k) & 1023u) << 8;
    d[2 + 2 * k] = lo;
    d[3 + 2 * k] = lo + len;
  }
}

}  // namespace gck
