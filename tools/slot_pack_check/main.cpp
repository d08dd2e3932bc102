// A stand-alone check of gochugaru_amd/csrc/slot_pack.hpp (the packing of an over-full user's cover
// entries into its slot) against brute force, meant to be built with the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I gochugaru_amd/csrc tools/slot_pack_check/main.cpp -o tools/slot_pack_check/slot_pack_check
//   tools/slot_pack_check/slot_pack_check
//
// Random entry sets of 1-64 raw entries (duplicates, dense blocks, both ends of the range) at both
// entry widths: the packed slot's inline entries and omitted run together are the sorted unique
// set, the run's open range is the narrowest, and every omitted entry lies strictly inside it.
// Then the 16-B resource fronts: what packs, what is flagged, and the round trip.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "slot_pack.hpp"

using namespace gck;

static uint32_t entry(uint32_t bits, const uint32_t* w, uint32_t k) {
  if (bits == 32) return w[1 + k];
  const uint32_t off = 32 + 24 * k, wi = off / 32, sh = off % 32;
  uint64_t v = w[wi] >> sh;
  if (sh + 24 > 32) v |= (uint64_t)w[wi + 1] << (32 - sh);
  return (uint32_t)(v & 0xFFFFFFu);
}

#define REQUIRE(c)                                                     \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::fprintf(stderr, "line %d: %s (case %d)\n", __LINE__, #c, it); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  std::mt19937_64 rng(12345);
  long listed = 0, fits = 0;
  for (int it = 0; it < 40000; ++it) {
    const uint32_t bits = it & 1 ? 24 : 32;
    const uint32_t cap = bits == 24 ? 20 : 15, n_in = cap - 2, unused = bits == 24 ? 0xFFFFFFu : 0xFFFFFFFFu;
    const uint32_t top = unused - 1;
    const uint32_t n = 1 + rng() % kSlotSortMax;
    std::vector<uint32_t> raw(n);
    const uint32_t base = (uint32_t)(rng() % (top - 300));
    for (uint32_t k = 0; k < n; ++k) {
      switch ((it >> 1) % 4) {
        case 0: raw[k] = (uint32_t)(rng() % (top + 1ull)); break;
        case 1: raw[k] = base + (uint32_t)(rng() % 300); break;
        case 2: raw[k] = (k & 1) ? (uint32_t)(rng() % 100) : top - (uint32_t)(rng() % 100); break;
        default: raw[k] = base + (uint32_t)(rng() % 30); break;
      }
    }
    std::vector<uint32_t> want = raw;
    std::sort(want.begin(), want.end());
    want.erase(std::unique(want.begin(), want.end()), want.end());
    std::vector<uint32_t> e = raw;  // (exactly n words: the sort may not step outside them)
    const uint32_t m = slot_sort_unique(e.data(), n);
    REQUIRE(m == want.size() && std::equal(want.begin(), want.end(), e.begin()));
    uint32_t w[kUSlotWords];
    slot_pack_sorted(bits, e.data(), m, 0xABCD0123u, w);
    if (m <= cap) {
      ++fits;
      REQUIRE(w[0] == m);
      for (uint32_t k = 0; k < cap; ++k) REQUIRE(entry(bits, w, k) == (k < m ? want[k] : unused));
      continue;
    }
    ++listed;
    const uint32_t n_om = m - n_in, s = slot_window(e.data(), m, n_in);
    REQUIRE(s <= n_in && (w[0] & kSlotList) && !(w[0] & kSlotOverflow) && slot_list_count(w[0]) == m);
    REQUIRE(slot_list_off(w) == 0xABCD0123u);
    REQUIRE(((w[0] & kSlotLoOpen) != 0) == (s == 0) && ((w[0] & kSlotHiOpen) != 0) == (s == n_in));
    auto width = [&](uint32_t k) {
      const uint32_t lo1 = k ? want[k - 1] + 1u : 0u, hi = k + n_om < m ? want[k + n_om] : 0xFFFFFFFFu;
      return hi - lo1;
    };
    for (uint32_t k = 0; k <= n_in; ++k) REQUIRE(width(s) <= width(k));
    std::vector<uint32_t> in(n_in);
    for (uint32_t k = 0; k < n_in; ++k) in[k] = entry(bits, w, k);
    if (s < n_in) REQUIRE(in[0] == want[s + n_om]);
    if (s > 0) REQUIRE(in[n_in - 1] == want[s - 1]);
    for (uint32_t k = s; k < s + n_om; ++k) {
      if (s > 0) REQUIRE(want[k] > in[n_in - 1]);
      if (s < n_in) REQUIRE(want[k] < in[0]);
    }
    std::sort(in.begin(), in.end());
    std::vector<uint32_t> rest(want.begin(), want.begin() + s);
    rest.insert(rest.end(), want.begin() + s + n_om, want.end());
    REQUIRE(in == rest);
    slot_pack_plain_list(bits, 65u + (uint32_t)(rng() % 1000), 7u, w);
    REQUIRE((w[0] & (kSlotLoOpen | kSlotHiOpen)) == (kSlotLoOpen | kSlotHiOpen) && slot_list_off(w) == 7u);
    for (uint32_t k = 0; k < n_in; ++k) REQUIRE(entry(bits, w, k) == unused);
  }
  // resource fronts: random slots of 0-7 intervals with lengths around the 18-bit edge; a front
  // packs exactly when the slot has at most 3 intervals that all fit, and then unpacks to the
  // slot's first eight words
  long packed = 0, flagged = 0;
  for (int it = 0; it < 40000; ++it) {
    uint32_t d[16] = {}, f[kFrontWords], u[8];
    const uint32_t n = (uint32_t)(rng() % 8);
    bool fit = n <= kFrontV;
    d[0] = n;
    for (uint32_t k = 0; k < n && k < 7; ++k) {
      const uint32_t lo = (uint32_t)(rng() % (1u << 24)) + ((rng() % 16 == 0) ? 1u << 24 : 0u);
      const uint32_t edge[] = {0u, 1u, 255u, 256u, kFrontLenMax - 1, kFrontLenMax, kFrontLenMax + 1, 1u << 20};
      const uint32_t len = rng() % 2 ? edge[rng() % 8] : 1u + (uint32_t)(rng() % kFrontLenMax);
      d[2 + 2 * k] = lo, d[3 + 2 * k] = lo + len;
      fit = fit && lo < (1u << 24) && len >= 1 && len <= kFrontLenMax;
    }
    if (it % 50 == 0) d[0] = kSlotOverflow, fit = false;
    const bool ok = front_pack(d, f);
    REQUIRE(ok == !front_flagged(f));
    bool all_ones = n == 3;  // (the one packed form that reads as the flag)
    for (uint32_t k = 0; k < 3 && all_ones; ++k) all_ones = d[2 + 2 * k] == 0xFFFFFFu && d[3 + 2 * k] - d[2 + 2 * k] == kFrontLenMax;
    REQUIRE(ok == (fit && !all_ones));
    if (!ok) {
      ++flagged;
      continue;
    }
    ++packed;
    front_unpack(f, u);
    for (uint32_t k = 0; k < 8; ++k) REQUIRE(u[k] == d[k]);
  }
  std::printf("slot_pack ok: %ld listed, %ld inline; fronts: %ld packed, %ld flagged\n", listed, fits, packed, flagged);
  return listed > 5000 && fits > 5000 && packed > 2000 && flagged > 5000 ? 0 : 1;
}
