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

}  // namespace gf
