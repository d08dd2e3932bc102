// select_plane.hpp — the ordered selection over a plane of 2-bit results (include/gck.h
// gck_filter_list_device): which checks of a 64-bit word survive a mask of Permissionships, how many
// survive in a run of words, and the records of a word's survivors at their ranks. Plain C++ that
// host code compiles as well as the device (k_dc_select in device_compact.inc calls it; gck_api.cpp
// exports it for the tests as gck_test_select_plane). Below them, the row-segmented form over a cross
// request's row-padded plane (gck_filter_cross_device; k_dc_rows_count / k_dc_rows_write, and
// gck_test_select_rows on the host), and its mirror, the column-segmented form
// (gck_filter_cross_cols_device; k_dc_cols_count / k_dc_cols_write, gck_test_select_cols). Last, the
// group-segmented form over a dense plane cut by caller-given offsets, and the group lookup of its
// pair expansion (gck_filter_groups_device; k_dc_group_pairs, k_dc_groups_count / k_dc_groups_write,
// gck_test_group_of and gck_test_select_groups). At the end, the selection over two planes of one
// request: the checks whose value changed from the old plane to the new one (gck_recheck_list_device,
// gck_recheck_cross_device; k_dc_diff, k_dc_diff_rows_count / k_dc_diff_rows_write, gck_test_change_plane
// and gck_test_change_rows).
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

// ---- the row-segmented selection over a cross plane (include/gck.h gck_filter_cross_device) ----
// The plane is S rows of `stride` = ceil(R / 32) words; row s keeps its first kept_s survivors, at
// ranks row_off[s] + j of the request. The kernels (k_dc_rows_count, k_dc_rows_write) and the host
// hook (gck_test_select_rows) walk a row in pieces of kRowPiece words, one word per lane of a wave.

constexpr uint32_t kRowPiece = 64;  // words of a row a wave takes at once

// The lanes of a wave that one row of `stride` words takes: the smallest power of two >= stride,
// within 1 .. 64 (a wave carries 64 / L rows; a longer row takes the whole wave, piece after piece).
GCK_SEL_HD inline uint32_t select_row_lanes(uint32_t stride) {
  uint32_t l = 1;
  while (l < stride && l < kRowPiece) l <<= 1;
  return l;
}

// What a row keeps of its surv survivors under row_limit (0: all of them).
GCK_SEL_HD inline uint32_t select_row_kept(uint32_t surv, uint32_t row_limit) {
  return row_limit && surv > row_limit ? row_limit : surv;
}

// The survivor mask of word t of a row of R checks: select_mask, with the padding lanes of the row's
// last word cleared (the engine writes them 0; a survivor's column is below R whatever they hold).
GCK_SEL_HD inline uint64_t select_row_mask(uint64_t word, uint32_t mask, uint32_t t, uint32_t R) {
  uint64_t m = select_mask(word, mask);
  const uint32_t col0 = t * 32u;
  if (col0 >= R) return 0;
  if (R - col0 < 32u) m &= (1ull << (2u * (R - col0))) - 1ull;
  return m;
}

// Where the kept survivors go: any of the three arrays may be null; `cap` entries each. A
// survivor's id is src_ids[r], r its column.
struct SelectRowsOut {
  uint32_t* ids;
  uint32_t* col;
  uint8_t* perm;
  uint32_t cap;
  const uint32_t* src_ids;
};

// The survivors m of one word of a row (word = its plane word, col0 = the column of its check 0), the
// first of them at in-row rank `rank`; the row's first record is at `row_base` of the request. Each is
// written while its in-row rank is below `limit` (0: no limit) and its rank in the request below
// cap. Ascending within the word.
GCK_SEL_HD inline void select_write_row(uint64_t word, uint64_t m, uint32_t col0, uint32_t rank, uint32_t row_base,
                                        uint32_t limit, const SelectRowsOut& o) {
  while (m) {
    if (limit && rank >= limit) return;
    const uint32_t at = row_base + rank;
    if (at >= o.cap) return;
    const uint32_t bit = (uint32_t)__builtin_ctzll(m);
    m &= m - 1u;
    const uint32_t r = col0 + (bit >> 1);
    if (o.ids) o.ids[at] = o.src_ids[r];
    if (o.col) o.col[at] = r;
    if (o.perm) o.perm[at] = (uint8_t)((word >> bit) & 3u);
    ++rank;
  }
}

// ---- the column-segmented selection over a cross plane (include/gck.h gck_filter_cross_cols_device) ----
// The mirror: column r of the same row-padded plane keeps its first kept_r survivors in ascending s,
// at ranks col_off[r] + j of the request. The kernels (k_dc_cols_count, k_dc_cols_write) and the host
// hook (gck_test_select_cols) give a column to a thread. A block has kColGroup columns — two
// word-columns of the plane — and takes the S rows in tiles of kColTile rows, whose two words per row
// it stages in LDS with one coalesced read; a tile is cut into kColChunks chunks of consecutive rows,
// one per wave. A thread counts its column in its chunk; the chunks before it (summed through LDS) and
// the tiles before (a running count) are its carried in-column rank, and it then walks its chunk
// downward writing records — ordered by construction, no atomics and no lane exchange.

constexpr uint32_t kColGroup = 64;    // columns of a block: one per lane of a wave (two word-columns)
constexpr uint32_t kColChunks = 16;   // row chunks of a tile: one per wave
constexpr uint32_t kColTile = 2048;   // rows of a tile (an in-place plane, at most 2,048 words, is one tile)
constexpr uint32_t kColBatch = 8;     // words a thread reads before it looks at them

// The rows of one chunk of a tile of T rows: the chunks are [k * n, min(T, (k + 1) * n)), the last
// ones empty when T is small.
GCK_SEL_HD inline uint32_t select_col_chunk_rows(uint32_t T) { return (T + kColChunks - 1u) / kColChunks; }

// Column c of a row of R checks, `word` the row's word c / 32: its GCK_PERM_* when it survives
// `mask`, else 0. Agrees with bit 2 (c % 32) of select_row_mask(word, mask, c / 32, R): a padding
// column of the row's last word (c >= R) never survives, whatever the plane holds there.
GCK_SEL_HD inline uint32_t select_col_perm(uint64_t word, uint32_t mask, uint32_t c, uint32_t R) {
  const uint32_t v = (uint32_t)(word >> (2u * (c & 31u))) & 3u;
  return c < R && ((mask >> v) & 1u) ? v : 0u;
}

// Where the kept survivors go: any of the three arrays may be null; `cap` entries each. A
// survivor's id is src_ids[s], s its row.
struct SelectColsOut {
  uint32_t* ids;
  uint32_t* row;
  uint8_t* perm;
  uint32_t cap;
  const uint32_t* src_ids;
};

// The record of the survivor in row s (perm: its GCK_PERM_*) at rank `at` of the request; at < cap.
GCK_SEL_HD inline void select_write_col(uint32_t s, uint32_t perm, uint32_t at, const SelectColsOut& o) {
  if (o.ids) o.ids[at] = o.src_ids[s];
  if (o.row) o.row[at] = s;
  if (o.perm) o.perm[at] = (uint8_t)perm;
}

// One chunk of one column as a thread walks it: rows s0 .. s0 + n - 1, the column's word of row
// s0 + i at words[i * step] (the staged tile on the device, the plane itself on the host), in batches
// of kColBatch words read first and looked at after. Returns the survivors met.
// With `o` the survivors are also written: the first of the chunk has in-column rank `rank`, the
// column's records start at `base` of the request and it keeps `kept` of its survivors; the walk ends
// at the first survivor beyond `kept` or beyond cap (ranks ascend, so every later one is beyond too).
GCK_SEL_HD inline uint32_t select_col_walk(const uint64_t* words, size_t step, uint32_t R, uint32_t mask, uint32_t c,
                                           uint32_t s0, uint32_t n, const SelectColsOut* o, uint32_t rank, uint32_t base,
                                           uint32_t kept) {
  uint32_t met = 0;
  for (uint32_t i = 0; i < n; i += kColBatch) {  // (n <= kColTile: i never wraps)
    uint64_t w[kColBatch];
#pragma unroll
    for (uint32_t k = 0; k < kColBatch; ++k) w[k] = k < n - i ? words[(size_t)(i + k) * step] : 0ull;  // (0: never survives)
#pragma unroll
    for (uint32_t k = 0; k < kColBatch; ++k) {
      const uint32_t v = select_col_perm(w[k], mask, c, R);
      if (!v) continue;
      ++met;
      if (!o) continue;
      if (rank >= kept || base + rank >= o->cap) return met;
      select_write_col(s0 + i + k, v, base + rank, *o);
      ++rank;
    }
  }
  return met;
}

// ---- the group-segmented selection over a dense plane (include/gck.h gck_filter_groups_device) ----
// The plane is the uniform request's: check k in bits 2 (k % 32) of word k / 32, ceil(n / 32) words.
// Group s owns the checks [off[s], off[s + 1]) — the words lo / 32 .. (hi - 1) / 32, the first and
// the last masked to the group's bits; two groups may share a word, and each reads it — and keeps its
// first kept_s survivors at ranks row_off[s] + j of the request. The offsets are the caller's device
// memory, which nobody has validated when the kernels read them: every function below stays inside
// [0, S - 1] and [0, n] whatever they hold. The kernels (k_dc_groups_count, k_dc_groups_write) and the
// host hook (gck_test_select_groups) give a group L lanes of a wave and walk it in pieces of L words.

// The group of check k: the last s in [0, S - 1] with off[s] <= k — for good offsets and k < n,
// off[s] <= k < off[s + 1], the group an upper-bound search of k in off[0 .. S] ends before. S >= 1.
// Reads off[1 .. S - 1] only; on offsets in no order the search still ends, somewhere in [0, S - 1].
GCK_SEL_HD inline uint32_t select_group_of(const uint32_t* off, uint32_t S, uint32_t k) {
  uint32_t lo = 0, hi = S - 1u;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1u) / 2u;  // (lo < mid <= hi)
    if (off[mid] <= k) lo = mid;
    else hi = mid - 1u;
  }
  return lo;
}

// Group s's checks [lo, hi), clamped into the request: lo = min(off[s], n), hi = min(max(off[s + 1],
// lo), n). n == 0 reads no offset.
GCK_SEL_HD inline void select_group_range(const uint32_t* off, uint32_t s, uint32_t n, uint32_t& lo, uint32_t& hi) {
  lo = hi = 0;
  if (n == 0) return;
  const uint32_t a = off[s], b = off[s + 1u];
  lo = a < n ? a : n;
  hi = b > lo ? b : lo;
  if (hi > n) hi = n;
}

// The lanes of a wave one group takes in a request of n checks in S groups: the smallest power of two
// >= ceil(n / S / 32) + 1 (an average group's words, and one more for a group that begins inside a
// word), within 1 .. 64. A longer group takes pieces of L words, with a carried rank.
GCK_SEL_HD inline uint32_t select_group_lanes(uint32_t n, uint32_t S) {
  const uint32_t per = S ? (uint32_t)(((uint64_t)n + S - 1u) / S) : 0u;
  const uint32_t want = (per + 31u) / 32u + 1u;
  uint32_t l = 1;
  while (l < want && l < 64u) l <<= 1;
  return l;
}

// The survivor mask of plane word t for the group [lo, hi): select_mask, with the checks below lo and
// at or above hi cleared. A word outside the group's words gives 0.
GCK_SEL_HD inline uint64_t select_group_mask(uint64_t word, uint32_t mask, uint32_t t, uint32_t lo, uint32_t hi) {
  const uint64_t k0 = (uint64_t)t * 32u;
  if (hi <= k0 || lo >= k0 + 32u || lo >= hi) return 0;
  uint64_t m = select_mask(word, mask);
  if (lo > k0) m &= ~((1ull << (2u * (uint32_t)(lo - k0))) - 1ull);
  if (hi < k0 + 32u) m &= (1ull << (2u * (uint32_t)(hi - k0))) - 1ull;
  return m;
}

// A group's kept survivors are written by select_write_row: SelectRowsOut with the candidate list as
// src_ids and the positions as `col`, col0 = 32 t — a survivor's column is its position k in the
// request, its id candidates[k].

// ---- the selection over two planes (include/gck.h gck_recheck_list_device, gck_recheck_cross_device) ----
// Two planes of one request, the caller's previous one and the one just written: check b of a word
// changed when its 2-bit fields differ, from v in the old word to w in the new one. `transitions` has
// bit 4 v + w set when that pair is selected (GCK_CHANGE_*; the diagonal bits 4 v + v are never set).
// Value 0 — an errored check — is a legal end of a transition. The change mask keeps select_mask's
// spacing, so a count is one popcount and the kernels are the selection kernels over two words.
// The old plane is the caller's memory: the padding lanes of a row's last word, or of a dense plane's
// last word, may hold anything in either plane, so every reader clears them (change_row_mask,
// change_tail_mask) and a change's column or position is below R or n whatever they hold.

constexpr uint32_t kChangeAny = 0x7BDEu;  // every off-diagonal pair (GCK_CHANGE_ANY)

// Bit 2b set: check b went from v to w, v != w, and `transitions` selects (v, w).
GCK_SEL_HD inline uint64_t change_mask(uint64_t old_word, uint64_t new_word, uint32_t transitions) {
  const uint64_t k = 0x5555555555555555ull;
  const uint64_t oe = old_word & k, oo = (old_word >> 1) & k, ne = new_word & k, no = (new_word >> 1) & k;
  const uint64_t ov[4] = {~oe & ~oo & k, oe & ~oo, oo & ~oe, oo & oe};
  const uint64_t nv[4] = {~ne & ~no & k, ne & ~no, no & ~ne, no & ne};
  uint64_t m = 0;
#pragma unroll
  for (uint32_t v = 0; v < 4u; ++v)
#pragma unroll
    for (uint32_t w = 0; w < 4u; ++w)
      if (v != w && ((transitions >> (4u * v + w)) & 1u)) m |= ov[v] & nv[w];
  return m;
}

// The change mask of word t of a row of R checks: change_mask, with the padding lanes of the row's
// last word cleared.
GCK_SEL_HD inline uint64_t change_row_mask(uint64_t old_word, uint64_t new_word, uint32_t transitions, uint32_t t,
                                           uint32_t R) {
  const uint32_t col0 = t * 32u;
  if (col0 >= R) return 0;
  uint64_t m = change_mask(old_word, new_word, transitions);
  if (R - col0 < 32u) m &= (1ull << (2u * (R - col0))) - 1ull;
  return m;
}

// The change mask of word t of a dense plane of n checks: change_mask, with the lanes at or beyond n
// cleared (t < 2^27: a plane of fewer than 2^32 checks).
GCK_SEL_HD inline uint64_t change_tail_mask(uint64_t old_word, uint64_t new_word, uint32_t transitions, uint32_t t,
                                            uint32_t n) {
  return change_row_mask(old_word, new_word, transitions, t, n);
}

// The changes of words begin, begin + stride, ... below `end` of a dense plane of n checks (old: null
// reads as zeros): select_count_strided over two planes.
GCK_SEL_HD inline uint32_t change_count_strided(const uint64_t* old_words, const uint64_t* new_words, uint32_t begin,
                                                uint32_t end, uint32_t stride, uint32_t transitions, uint32_t n) {
  uint32_t c = 0;
  for (uint32_t t = begin; t < end; t += stride)
    c += select_count(change_tail_mask(old_words ? old_words[t] : 0ull, new_words[t], transitions, t, n));
  return c;
}

// A change's transition byte: 4 * old + new, its bit index in `transitions`.
GCK_SEL_HD inline uint8_t change_byte(uint64_t old_word, uint64_t new_word, uint32_t bit) {
  return (uint8_t)(4u * ((uint32_t)(old_word >> bit) & 3u) + ((uint32_t)(new_word >> bit) & 3u));
}

// Where the dense form's records go: SelectOut with the transition byte in place of the value.
struct ChangeOut {
  uint32_t* ids;
  uint32_t* pos;
  uint8_t* trans;
  uint32_t cap;
  const uint32_t* src_ids;
  uint32_t first_id, pos0;
};

// The changes m of word t of the chunk, the first of them at `rank` of the request: each is written
// while its rank is below cap. Ascending within the word.
GCK_SEL_HD inline void change_write(uint64_t old_word, uint64_t new_word, uint64_t m, uint32_t t, uint32_t rank,
                                    const ChangeOut& o) {
  while (m && rank < o.cap) {
    const uint32_t bit = (uint32_t)__builtin_ctzll(m);
    m &= m - 1u;
    const uint32_t i = t * 32u + (bit >> 1);
    if (o.ids) o.ids[rank] = o.src_ids ? o.src_ids[i] : o.first_id + i;
    if (o.pos) o.pos[rank] = o.pos0 + i;
    if (o.trans) o.trans[rank] = change_byte(old_word, new_word, bit);
    ++rank;
  }
}

// Where the row form's records go: a change's id is src_ids[r], r its column.
struct ChangeRowsOut {
  uint32_t* ids;
  uint32_t* col;
  uint8_t* trans;
  uint32_t cap;
  const uint32_t* src_ids;
};

// The changes m of one word of a row (col0 = the column of its check 0), the first of them at in-row
// rank `rank`; the row's first record is at `row_base` of the request. Each is written while its rank
// in the request is below cap. Ascending within the word.
GCK_SEL_HD inline void change_write_row(uint64_t old_word, uint64_t new_word, uint64_t m, uint32_t col0, uint32_t rank,
                                        uint32_t row_base, const ChangeRowsOut& o) {
  while (m) {
    const uint32_t at = row_base + rank;
    if (at >= o.cap) return;
    const uint32_t bit = (uint32_t)__builtin_ctzll(m);
    m &= m - 1u;
    const uint32_t r = col0 + (bit >> 1);
    if (o.ids) o.ids[at] = o.src_ids[r];
    if (o.col) o.col[at] = r;
    if (o.trans) o.trans[at] = change_byte(old_word, new_word, bit);
    ++rank;
  }
}

}  // namespace gck
