// Stand-alone check of the compacted drain's helpers in csrc/net_delta.h (built by
// tests/test_net_compact_cpu.py with the host compiler). It plays one wave's batch the way
// store_network_rows_delta does: lane l holds record word l, derives its four group flags,
// the dirty groups are listed one byte each at the slots the four masks give, and the drain
// hands entry 16 it + (l >> 2), float4 l & 3 to lane l. The float4s so stored must be
// exactly those of the groups that net_group_dirty<64> calls dirty: each once, none outside
// its row, no slot past 255, each with the row's own 4 adjacency bits.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "net_delta.h"

namespace {

uint64_t splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

enum Kind { kRandom, kSparse, kClean, kAllDirty, kSingle, kValueOnly, kForced, kKinds };

struct Batch {
  int Wn, N;     // words and columns of a row
  int nrb;       // rows in the batch
  int cw0, cnt;  // first word of the rows' columns in the batch, words in the batch
};

long bad = 0, batches = 0, stored = 0, max_slot = -1;

void fail(const char* what, const Batch& b, int kind, long a = 0, long c = 0) {
  if (bad < 20)
    std::printf("FAIL %s: Wn=%d N=%d nrb=%d cw0=%d cnt=%d kind=%d (%ld, %ld)\n", what, b.Wn, b.N, b.nrb, b.cw0, b.cnt,
                kind, a, c);
  ++bad;
}

// the valid bits of word cw of a row of N columns
uint64_t valid_bits(int N, int cw) {
  const int left = N - cw * 64;
  return left >= 64 ? ~0ull : (left <= 0 ? 0ull : ((1ull << left) - 1ull));
}

void run_batch(const Batch& b, int kind, uint64_t& seed) {
  const bool rows_form = b.Wn <= 64;  // whole rows per batch, else a chunk of one row
  const int nq = b.N >> 2;
  const uint32_t rdiv = gf::net_compact_rdiv(b.Wn);
  const bool force = kind == kForced;
  // the batch's words: word w is word (w % Wn) of row (w / Wn), or word cw0 + w of the row
  std::vector<uint64_t> oldw(64, 0), neww(64, 0);
  std::vector<int> vc(b.nrb, 0);
  const int single = static_cast<int>(splitmix(seed) % (b.cnt * 4));
  for (int r = 0; r < b.nrb; ++r) vc[r] = (kind == kRandom || kind == kSparse) ? (splitmix(seed) & 1) : (kind == kValueOnly);
  for (int w = 0; w < b.cnt; ++w) {
    const int cw = rows_form ? w % b.Wn : b.cw0 + w;
    const uint64_t vb = valid_bits(b.N, cw);
    uint64_t o = splitmix(seed) & splitmix(seed), n = o;
    switch (kind) {
      case kRandom: n = splitmix(seed) & splitmix(seed); break;
      case kSparse:
        if ((splitmix(seed) & 3) == 0) n = o ^ (1ull << (splitmix(seed) & 63));
        break;
      case kAllDirty: n = ~o; break;
      case kSingle:
        if (w == single >> 2) n = o ^ (1ull << (16 * (single & 3)));  // (may fall past the row's end: then clean)
        break;
      default: break;  // kClean, kValueOnly, kForced: the same bits
    }
    oldw[w] = o & vb;
    neww[w] = n & vb;
  }
  // lanes: flags, masks
  uint32_t flags[64] = {};
  uint64_t qm[4] = {0, 0, 0, 0};
  for (int l = 0; l < 64; ++l) {
    const int lrow = static_cast<int>((static_cast<uint32_t>(l) * rdiv) >> 16);
    if (lrow != (rows_form ? l / b.Wn : 0)) fail("lane row", b, kind, l, lrow);
    if (l >= b.cnt) continue;
    const uint64_t x = force ? ~0ull : (oldw[l] ^ neww[l]);
    flags[l] = gf::net_word_flags(x, neww[l], force || vc[lrow] != 0);
    for (int k = 0; k < 4; ++k)
      if ((flags[l] >> k) & 1u) qm[k] |= 1ull << l;
  }
  int D = 0;
  for (int k = 0; k < 4; ++k) D += __builtin_popcountll(qm[k]);
  // the list
  int ent[gf::kNetCompactSlots];
  std::fill(ent, ent + gf::kNetCompactSlots, -1);
  for (int l = 0; l < b.cnt; ++l)
    for (int k = 0; k < 4; ++k)
      if ((flags[l] >> k) & 1u) {
        const int slot = gf::net_compact_slot(qm, k, l);
        max_slot = std::max<long>(max_slot, slot);
        if (slot < 0 || slot >= gf::kNetCompactSlots || slot >= D) {
          fail("slot out of range", b, kind, slot, D);
          continue;
        }
        if (ent[slot] != -1) fail("slot used twice", b, kind, slot);
        const uint32_t e = gf::net_compact_entry(l, k);
        if (e > 255u) fail("entry is not a byte", b, kind, e);
        ent[slot] = static_cast<int>(e);
      }
  for (int i = 0; i < D; ++i)
    if (ent[i] == -1) fail("hole in the list", b, kind, i, D);
  // the group's 16 new bits as the kernel reads them: half-word `entry` of the batch's words
  uint16_t a16[256];
  for (int w = 0; w < 64; ++w)
    for (int k = 0; k < 4; ++k) a16[4 * w + k] = static_cast<uint16_t>(neww[w] >> (16 * k));
  // the drain
  std::vector<int> hits(static_cast<size_t>(b.nrb) * nq, 0);
  const int nit = (D + 15) >> 4;
  if (nit != (4 * D + 63) / 64) fail("iterations", b, kind, nit, D);
  for (int it = 0; it < nit; ++it)
    for (int l = 0; l < 64; ++l) {
      const int i = 16 * it + (l >> 2), f = l & 3;
      if (i >= D || ent[i] < 0) continue;
      const uint32_t e = static_cast<uint32_t>(ent[i]);
      const gf::NetCompactDst to = gf::net_compact_dst(e, f, b.Wn, rdiv, b.cw0, nq);
      const int w = static_cast<int>(e >> 2);
      const int want_row = rows_form ? w / b.Wn : 0;
      const int want_q = ((rows_form ? w % b.Wn : b.cw0 + w) << 4) + ((e & 3) << 2) + f;
      if (to.row != want_row || to.q != want_q || to.ok != (want_q < nq)) fail("destination", b, kind, e, f);
      if (!to.ok) continue;
      if (to.row < 0 || to.row >= b.nrb || to.q < 0 || to.q >= nq) {
        fail("store outside its row", b, kind, to.row, to.q);
        continue;
      }
      // the float4's adjacency bits: nibble f of the group's half-word = bits 4q..4q+3 of the row
      const unsigned nib = (a16[e] >> (4 * f)) & 0xFu;
      const int cw = to.q >> 4, wi = rows_form ? to.row * b.Wn + cw : cw - b.cw0;
      if (nib != ((neww[wi] >> ((to.q & 15) << 2)) & 0xFull)) fail("adjacency nibble", b, kind, to.row, to.q);
      ++hits[static_cast<size_t>(to.row) * nq + to.q];
      ++stored;
    }
  // against the definition, float4 by float4 of the batch's part of every row
  for (int r = 0; r < b.nrb; ++r)
    for (int q = 0; q < nq; ++q) {
      const int cw = q >> 4;
      const bool in_batch = rows_form || (cw >= b.cw0 && cw < b.cw0 + b.cnt);
      bool want = false;
      if (in_batch) {
        const int wi = rows_form ? r * b.Wn + cw : cw - b.cw0;
        const int bit = (q & 15) << 2, half = bit >> 5;
        const uint32_t o = static_cast<uint32_t>(oldw[wi] >> (32 * half)), n = static_cast<uint32_t>(neww[wi] >> (32 * half));
        want = force || gf::net_group_dirty<64>(gf::net_delta_bits(o ^ n, n, vc[r] != 0), bit & 31);
      }
      if (hits[static_cast<size_t>(r) * nq + q] != (want ? 1 : 0)) fail("stored float4s", b, kind, r, q);
    }
  if (kind == kClean && D != 0) fail("clean batch has entries", b, kind, D);
  if (kind == kAllDirty && rows_form && b.N == b.Wn * 64 && D != 4 * b.cnt) fail("all-dirty batch", b, kind, D);
  ++batches;
}

}  // namespace

int main() {
  uint64_t seed = 20250711ull;
  const int wns[] = {1, 2, 3, 16, 17, 64, 65, 128};
  for (int Wn : wns)
    for (int c = 4; c <= 64; c += 4) {  // every N % 4 == 0 of this Wn: N % 16 in {0, 4, 8, 12}
      const int N = (Wn - 1) * 64 + c;
      std::vector<Batch> forms;
      if (Wn <= 64) {
        const int rpb = 64 / Wn;
        for (int nrb : {rpb, 1, (rpb + 1) / 2})  // a full batch and the shorter last ones
          forms.push_back(Batch{Wn, N, nrb, 0, nrb * Wn});
      } else {
        for (int cw0 = 0; cw0 < Wn; cw0 += 64) forms.push_back(Batch{Wn, N, 1, cw0, std::min(64, Wn - cw0)});
      }
      for (const Batch& b : forms)
        for (int kind = 0; kind < kKinds; ++kind)
          for (int rep = 0; rep < ((kind == kRandom || kind == kSparse || kind == kSingle) ? 8 : 1); ++rep)
            run_batch(b, kind, seed);
    }
  std::printf("net_compact_check: batches=%ld stored=%ld max_slot=%ld bad=%ld\n", batches, stored, max_slot, bad);
  return bad == 0 ? 0 : 1;
}
