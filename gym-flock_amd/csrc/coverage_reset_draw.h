// cov_reset_device's draws for one env by one wave (coverage_reset.hip has the account of
// them), as a device function: cov_reset_draw_kernel runs it in a workgroup of one wave, and
// cov_rollout_kernel (coverage_rollout.hip) in wave 0 of an env's workgroup when an episode
// ends inside a launch, so both run the same code.
#pragma once
#include "coverage_internal.h"

namespace gf {

// The draws of env b, entry e of the launch's list. smem: the draw's LDS
// (cov_reset_draw_lds_bytes). Every lane of the wave calls it with threadIdx.x its lane.
// Sync (mt19937.h): how the wave orders its LDS accesses. Returns the status bits.
// ROLL (the rollout): the stream always continues, and of the outputs only the start row, the
// visited row and the stream are written; the status is the return value alone.
template <bool ROLL, class Sync>
__device__ __forceinline__ int cov_reset_draw_body(const CovResetDrawArgs& a, const int e, const int b,
                                                   unsigned char* smem) {
  const Sync sync;
  const int lane = threadIdx.x;
  const int R = a.R, Tm = a.Tmax, T = min(a.ntg[b], Tm);
  const int W = ((Tm + 63) / 64) * 2;  // words per bit set
  uint32_t* key = reinterpret_cast<uint32_t*>(smem);
  int32_t* perm = reinterpret_cast<int32_t*>(key + kMtN);
  int32_t* vseq = perm + Tm;
  uint32_t* reg = reinterpret_cast<uint32_t*>(vseq + Tm);  // the region
  uint32_t* nxt = reg + W;                                 // the region after this round
  uint8_t* vis = reinterpret_cast<uint8_t*>(nxt + W);
  int pos;  // wave-uniform
  if (!ROLL && a.seed) {
    if (lane == 0) {
      uint32_t s = a.seed0 + static_cast<uint32_t>(b);
      for (int p = 0; p < kMtN; ++p) {
        key[p] = s;
        s = 1812433253u * (s ^ (s >> 30)) + static_cast<uint32_t>(p + 1);
      }
    }
    pos = kMtN;
  } else {
    for (int k = lane; k < kMtN; k += 64) key[k] = a.mt_key[(size_t)b * kMtN + k];
    pos = min(max(a.mt_pos[b], 0), kMtN);
  }
  for (int w = lane; w < W; w += 64) reg[w] = nxt[w] = 0u;
  sync();
  int status = 0, nreg = T;
  if (a.nearby > 0) {
    // 1. i = choice(T)
    int i0 = 0;
    if (T > 1) {
      const uint32_t top = static_cast<uint32_t>(T - 1);
      const uint32_t mask = 0xFFFFFFFFu >> __builtin_clz(top);
      for (;;) {
        if (pos == kMtN) {
          mt_regen<64, Sync>(key);
          pos = 0;
        }
        const uint32_t v = mt_temper(key[pos]) & mask;  // every lane reads the same word
        ++pos;
        if (v <= top) {
          i0 = static_cast<int>(v);
          break;
        }
      }
    }
    // 2. the region
    if (lane == 0) reg[i0 >> 5] = nxt[i0 >> 5] = 1u << (i0 & 31);
    sync();
    const int32_t* nbr = a.nbr + (size_t)b * Tm * 4;
    const int32_t* cnt = a.cnt + (size_t)b * Tm;
    nreg = 1;
    while (nreg < a.nearby) {
      for (int t = lane; t < T; t += 64) {
        if (!((reg[t >> 5] >> (t & 31)) & 1u)) continue;
        const int c = min(cnt[t], 4);
        const int4 q = *reinterpret_cast<const int4*>(nbr + 4 * t);
        const int qv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < c && qv[k] >= 0 && qv[k] < T) atomicOr(&nxt[qv[k] >> 5], 1u << (qv[k] & 31));
      }
      sync();
      int n = 0;
      for (int w = lane; w < W; w += 64) {
        const uint32_t v = nxt[w];
        reg[w] = v;
        n += __popc(v);
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
      sync();
      if (n == nreg) {
        status |= kResetRegionShort;
        break;
      }
      nreg = n;
    }
  } else {
    for (int t = lane; t < T; t += 64) atomicOr(&reg[t >> 5], 1u << (t & 31));
    sync();
  }
  if constexpr (!ROLL) {
    uint8_t* region = a.region + (size_t)b * Tm;
    for (int t = lane; t < Tm; t += 64) {
      const uint8_t in = (t < T && ((reg[t >> 5] >> (t & 31)) & 1u)) ? 1 : 0;
      region[t] = in;
      if (a.region_c) a.region_c[(size_t)e * Tm + t] = in;
    }
  }
  if (nreg < R || T < R) {
    // 3'. choice(members, R, replace=False) raises before it draws: the env is not reset
    // (the reset pass skips it; its start row reads -1, its visited row 1)
    status |= kResetRegionSmall;
    for (int k = lane; k < R; k += 64) {
      a.start[(size_t)b * R + k] = -1;
      if (!ROLL && a.start_c) a.start_c[(size_t)e * R + k] = -1;
    }
    for (int t = lane; t < Tm; t += 64) {
      a.visited0[(size_t)b * Tm + t] = 1;
      if (!ROLL && a.visited_c) a.visited_c[(size_t)e * Tm + t] = 1;
    }
  } else {
    // 3. the start targets
    cov_permute<Sync>(key, pos, perm, vseq, nreg);
    int run = 0;  // the members in ascending order into vseq (free between permutations)
    for (int t0 = 0; t0 < T; t0 += 64) {
      const int t = t0 + lane;
      const bool in = t < T && ((reg[t >> 5] >> (t & 31)) & 1u);
      const uint64_t m = __ballot(in);
      const int at = run + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                     __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0));
      if (in) vseq[at] = t;
      run += __popcll(m);
    }
    sync();
    for (int k = lane; k < R; k += 64) {
      const int t = vseq[perm[k]];
      a.start[(size_t)b * R + k] = t;
      if (!ROLL && a.start_c) a.start_c[(size_t)e * R + k] = t;
    }
    sync();
    // 4. the unvisited targets
    cov_permute<Sync>(key, pos, perm, vseq, T);
    const int kdrop = static_cast<int>(static_cast<double>(T) * a.frac);  // Python's int(T * frac)
    for (int t = lane; t < Tm; t += 64) vis[t] = 1;
    sync();
    for (int k = lane; k < kdrop; k += 64) vis[perm[k]] = 0;
    sync();
    for (int t = lane; t < Tm; t += 64) {
      a.visited0[(size_t)b * Tm + t] = vis[t];
      if (!ROLL && a.visited_c) a.visited_c[(size_t)e * Tm + t] = vis[t];
    }
  }
  for (int k = lane; k < kMtN; k += 64) a.mt_key[(size_t)b * kMtN + k] = key[k];
  if (lane == 0) {
    a.mt_pos[b] = pos;
    if constexpr (!ROLL) {
      a.status[b] = status;
      a.nregion[b] = nreg;
      a.envs_ok[e] = (status & kResetRegionSmall) ? -1 : b;
    }
  }
  return status;
}

}  // namespace gf
