// Stand-alone check of csrc/net_delta.h (built by tests/test_net_delta_cpu.py with the
// host compiler): the group flags against their definition, spelled out bit by bit.
//   A group is stored when its new bits differ from its recorded bits, or when it has a
//   new bit set and the row's value changed.
#include <cstdint>
#include <cstdio>

#include "net_delta.h"

namespace {

// the definition, for the group of `w` adjacency bits starting at bit g0 of a 64-bit word
bool want_dirty(uint64_t old_w, uint64_t new_w, bool vc, int g0, int w) {
  bool differ = false, any_new = false;
  for (int k = g0; k < g0 + w; ++k) {
    const bool o = (old_w >> k) & 1u, n = (new_w >> k) & 1u;
    differ = differ || (o != n);
    any_new = any_new || n;
  }
  return differ || (any_new && vc);
}

// the helper's answer for adjacency bit `bit` (0..63) of the word, as the kernel asks it:
// by 32-bit halves
template <int G>
bool got_dirty(uint64_t old_w, uint64_t new_w, bool vc, int bit) {
  const int half = bit >> 5;
  const uint32_t o = static_cast<uint32_t>(old_w >> (32 * half)), n = static_cast<uint32_t>(new_w >> (32 * half));
  return gf::net_group_dirty<G>(gf::net_delta_bits(o ^ n, n, vc), bit & 31);
}

template <int G>
long check_word(uint64_t old_w, uint64_t new_w, bool vc) {
  long bad = 0;
  constexpr int W = G / 4;
  for (int bit = 0; bit < 64; bit += 4)  // every float4 of the word asks for its own group
    if (got_dirty<G>(old_w, new_w, vc, bit) != want_dirty(old_w, new_w, vc, bit & ~(W - 1), W)) ++bad;
  return bad;
}

uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

}  // namespace

int main() {
  long bad = 0, cases16 = 0, cases_wide = 0;
  // 16-byte groups: every (old nibble, new nibble, value changed), at every nibble of the
  // word, alone and with the rest of the word set in both (neighbours must not leak in)
  for (int pos = 0; pos < 64; pos += 4)
    for (unsigned o = 0; o < 16; ++o)
      for (unsigned n = 0; n < 16; ++n)
        for (int vc = 0; vc < 2; ++vc)
          for (int fill = 0; fill < 2; ++fill) {
            const uint64_t rest = fill ? ~(0xFull << pos) : 0ull;
            const uint64_t ow = (static_cast<uint64_t>(o) << pos) | rest, nw = (static_cast<uint64_t>(n) << pos) | rest;
            const bool want = (o != n) || (n != 0 && vc);
            if (got_dirty<16>(ow, nw, vc != 0, pos) != want) ++bad;
            // an unchanged, fully set neighbour is dirty exactly when the value changed
            if (fill && got_dirty<16>(ow, nw, vc != 0, (pos + 4) & 63) != (vc != 0)) ++bad;
            ++cases16;
          }
  // wider groups: seeded random words; sparse differences too, so clean groups occur
  uint64_t s = 20240607ull;
  for (int k = 0; k < 1000000; ++k) {
    const uint64_t ow = splitmix(s) & splitmix(s);
    uint64_t nw = splitmix(s) & splitmix(s);
    const uint64_t r = splitmix(s);
    const bool vc = r & 1u;
    switch ((r >> 1) & 3u) {
      case 0: nw = ow; break;                                   // nothing changed
      case 1: nw = ow ^ (1ull << ((r >> 8) & 63u)); break;      // one bit flipped
      case 2: nw = ow & ~(0xFFFFull << (((r >> 8) & 3u) * 16)); break;  // one 64-byte group emptied
      default: break;                                           // unrelated words
    }
    bad += check_word<16>(ow, nw, vc) + check_word<64>(ow, nw, vc) + check_word<128>(ow, nw, vc);
    ++cases_wide;
  }
  std::printf("net_delta_check: group=%d cases16=%ld cases_wide=%ld bad=%ld\n", gf::kNetGroupBytes, cases16, cases_wide, bad);
  return bad == 0 ? 0 : 1;
}
