// select_plane.hpp — the ordered selection over a plane of 2-bit results (include/gck.h
// gck_filter_list_device): which checks of a 64-bit word survive a mask of Permissionships, how many
// survive in a run of words, and the records of a word's survivors at their ranks. Plain C++ that
// host code compiles as well as the device (k_dc_select in device_compact.inc calls it; gck_api.cpp
// exports it for the tests as gck_test_select_plane).
//
// A word holds 32 checks, check b in bits 2b .. 2b + 1 (GCK_PERM_*: 0 unspecified — an errored check
// and a tail lane alike —, 1 NO, 2 HAS, 3 CONDITIONAL). `mask` has bit v set when value v survives
// (GCK_SELECT_*; bit 0 is never set, so a zero field never survives and the plane alone decides).
// The survivor mask keeps the plane's spacing: bit 2b is set when check b survives, every odd bit is
// 0 — 32 positions in 64 bits, so the count is one popcount and a survivor's field is found at the
// bit the walk stops on, without a compaction step.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GCK_SEL_HD __host__ __device__
#else
#define GCK_SEL_HD
#endif

namespace gck {

constexpr uint32_t kSelBlock = 256;  // words per tile: one per thread of a block of k_dc_select

// Bit 2b set: check b of `word` survives `mask`.
GCK_SEL_HD inline uint64_t select_mask(uint64_t word, uint32_t mask) {
  const uint64_t even = word & 0x5555555555555555ull, odd = (word >> 1) & 0x5555555555555555ull;
  uint64_t m = 0;
  if (mask & 2u) m |= even & ~odd;  // 1: NO
  if (mask & 4u) m |= odd & ~even;  // 2: HAS
  if (mask & 8u) m |= odd & even;   // 3: CONDITIONAL
  return m;
}

GCK_SEL_HD inline uint32_t select_count(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }

// The survivors of words[begin], words[begin + stride], ... below `end`: what a block counts again of
// the words before its tile (thread t: begin = t, stride = the block), and what one caller counts of
// a whole run (begin = 0, stride = 1).
GCK_SEL_HD inline uint32_t select_count_strided(const uint64_t* words, uint32_t begin, uint32_t end, uint32_t stride,
                                                uint32_t mask) {
  uint32_t c = 0;
  for (uint32_t t = begin; t < end; t += stride) c += select_count(select_mask(words[t], mask));
  return c;
}

// Where the survivors go: any of the three arrays may be null; `cap` entries each. A survivor's id
// is ids[i] of its chunk, or first_id + i without a list; its position is pos0 + i (pos0: the chunk's
// offset in the request).
struct SelectOut {
  uint32_t* ids;
  uint32_t* pos;
  uint8_t* perm;
  uint32_t cap;
  const uint32_t* src_ids;
  uint32_t first_id, pos0;
};

// The survivors m of word t of the chunk (word = its plane word), the first of them at `rank` of the
// request: each is written while its rank is below cap. Ascending within the word.
GCK_SEL_HD inline void select_write(uint64_t word, uint64_t m, uint32_t t, uint32_t rank, const SelectOut& o) {
  while (m && rank < o.cap) {
    const uint32_t bit = (uint32_t)__builtin_ctzll(m);
    m &= m - 1u;
    const uint32_t i = t * 32u + (bit >> 1);
    if (o.ids) o.ids[rank] = o.src_ids ? o.src_ids[i] : o.first_id + i;
    if (o.pos) o.pos[rank] = o.pos0 + i;
    if (o.perm) o.perm[rank] = (uint8_t)((word >> bit) & 3u);
    ++rank;
  }
}

}  // namespace gck
