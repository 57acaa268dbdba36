// Delta network store: which groups of a dense network row must be stored again, from
// the row's new adjacency bits, the bits the buffer's record holds and whether the row's
// value (1/deg) changed. Plain C++ outside hipcc (tests/test_net_delta_cpu.py builds a
// stand-alone program around it with the host compiler).
//
// A group is kNetGroupBytes of the row (4 floats per 16 bytes: 4, 16 or 32 adjacency
// bits, aligned from the row's start). It is stored when
//   - its new bits differ from its recorded bits, or
//   - it has a new bit set and the row's new value differs from the recorded one;
// every other group already holds what the step would write.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GF_ND_HD __host__ __device__ __forceinline__
#else
#define GF_ND_HD inline
#endif

namespace gf {

// Group size of the plain step's delta store: 16, 64 or 128 bytes ("Delta
// network store" has the three measured against each other).
#ifndef GF_NET_GROUP_BYTES
#define GF_NET_GROUP_BYTES 64
#endif
constexpr int kNetGroupBytes = GF_NET_GROUP_BYTES;
static_assert(kNetGroupBytes == 16 || kNetGroupBytes == 64 || kNetGroupBytes == 128, "group size");

// The bits of 32 adjacency bits that make their group dirty: x = recorded ^ new.
GF_ND_HD uint32_t net_delta_bits(uint32_t x, uint32_t nw, bool value_changed) {
  return x | (value_changed ? nw : 0u);
}

// Whether the group of G bytes that holds adjacency bit `bit` (0..31 of the word d =
// net_delta_bits(...)) must be stored.
template <int G>
GF_ND_HD bool net_group_dirty(uint32_t d, int bit) {
  constexpr int W = G / 4;  // adjacency bits per group
  static_assert(W == 4 || W == 16 || W == 32, "group size");
  if constexpr (W == 32)
    return d != 0u;
  else
    return ((d >> (bit & ~(W - 1))) & ((1u << W) - 1u)) != 0u;
}

// ---- Compacted drain (64-byte groups): a wave compares a batch of up to 64 record words
// (64 adjacency bits each: four groups, "quarters"), lists the dirty groups of the batch
// and stores them four lanes to a group, 16 groups to a wave instruction.
//
// A batch is either whole rows (Wn <= 64 words per row: word w of the batch is word
// w % Wn of the batch's row w / Wn) or a chunk of one row (Wn > 64: word w of the batch is
// word cw0 + w of the row).

constexpr int kNetCompactSlots = 256;  // 64 words x 4 quarters: one byte per list entry

// The four group flags of a record word: bit k set when quarter k (adjacency bits
// 16k..16k+15) must be stored. x = recorded ^ new, nw = new, vc = its row's value changed.
GF_ND_HD uint32_t net_word_flags(uint64_t x, uint64_t nw, bool vc) {
  const uint32_t dl = net_delta_bits(static_cast<uint32_t>(x), static_cast<uint32_t>(nw), vc);
  const uint32_t dh = net_delta_bits(static_cast<uint32_t>(x >> 32), static_cast<uint32_t>(nw >> 32), vc);
  return ((dl & 0xFFFFu) ? 1u : 0u) | ((dl >> 16) ? 2u : 0u) | ((dh & 0xFFFFu) ? 4u : 0u) | ((dh >> 16) ? 8u : 0u);
}

// A list entry: the batch's word and the quarter of it.
GF_ND_HD uint32_t net_compact_entry(int word, int quarter) { return (static_cast<uint32_t>(word) << 2) | quarter; }

// Bits of `m` below bit `lane`.
GF_ND_HD int net_lanes_below(uint64_t m, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
#else
  return __builtin_popcountll(m & ((1ull << lane) - 1ull));
#endif
}

// The slot of lane `lane`'s quarter k in the list, from the four masks m[k] = the lanes
// whose word has quarter k dirty: the quarters one after the other, lanes ascending.
// (The number of entries is the four masks' population.)
GF_ND_HD int net_compact_slot(const uint64_t m[4], int k, int lane) {
  int base = 0;
  for (int j = 0; j < k; ++j) base += __builtin_popcountll(m[j]);
  return base + net_lanes_below(m[k], lane);
}

// w / Wn for 0 <= w < 64 as (w * net_compact_rdiv(Wn)) >> 16: exact for 1 <= Wn <= 64 (the
// quotient's fraction is at most 1 - 1/Wn and the error below 64 / 65536), and 0 for every
// Wn >= 64: one expression maps an entry to its row in both batch forms.
GF_ND_HD uint32_t net_compact_rdiv(int Wn) { return (65536u + static_cast<uint32_t>(Wn) - 1u) / static_cast<uint32_t>(Wn); }

// Where float4 f (0..3) of a list entry goes: the row of the batch, the float4 column of
// that row, and whether it lies inside the row (nq = N / 4 float4s; a row's last word may
// hold fewer than four groups and its last group fewer than four float4s).
struct NetCompactDst {
  int row, q;
  bool ok;
};
GF_ND_HD NetCompactDst net_compact_dst(uint32_t entry, int f, int Wn, uint32_t rdiv, int cw0, int nq) {
  const int w = static_cast<int>(entry >> 2);
  NetCompactDst t;
  t.row = static_cast<int>((static_cast<uint32_t>(w) * rdiv) >> 16);
  t.q = ((cw0 + w - t.row * Wn) << 4) + (static_cast<int>(entry & 3u) << 2) + f;
  t.ok = t.q < nq;
  return t;
}

}  // namespace gf
