// cov_reset_device's draws (gfx950): reset()'s random draws (coverage.py:398-414, :596-599)
// of chosen envs from their own np_random streams, with the reference's nearby_starts
// region grown through the motion graph (get_n_nearest :655-673).
//
// One wave per selected env, the env taken from a device list: cov_seed_reset_kernel's
// scheme (coverage_kernels.hip) with its permutation (cov_permute, coverage_internal.h).
// The key comes from mt_key / mt_pos (or is seeded, COV_RESET_SEED), then in the
// reference's order:
//   1. nearby > 0: i = np_random.choice(T), a scalar draw: randint(0, T), numpy's masked
//      rejection on 32-bit words with the mask of T - 1 (T == 1 draws nothing);
//   2. the region as two bit sets in LDS, region = {i}; while |region| < nearby: region |=
//      out-neighbours(region), from the device's neighbour table nbr / cnt (the motion edge
//      list, at most 4 per node). A round expands the set as it stood at its start, may
//      overshoot nearby, and a round that adds nothing ends the loop (kResetRegionShort: the
//      reference would loop forever);
//   3. start = members_ascending[permutation(|region|)[:R]], the members compacted by
//      ballot prefix per 64 targets. Fewer members than robots: numpy raises before drawing
//      (kResetRegionSmall), the env is struck from the list (envs_ok) and only its stream
//      is written back;
//   4. unvisited = permutation(T)[:int(T * frac)].
// With nearby == 0 the members are all T targets and steps 3-4 are cov_seed_reset_kernel's.
//
// LDS: key (624 words), perm (Tmax words), vseq (Tmax words: a permutation's draws, then the
// region's members), the two bit sets (ceil(Tmax / 64) * 2 words each), the visited flags
// (Tmax bytes): cov_reset_draw_lds_bytes.
#include "coverage_internal.h"

namespace gf {

namespace {

__global__ __launch_bounds__(64) void cov_reset_draw_kernel(CovResetDrawArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= a.n_sel) return;
  const int b = a.envs[e];
  const int R = a.R, Tm = a.Tmax, T = min(a.ntg[b], Tm);
  const int W = ((Tm + 63) / 64) * 2;  // words per bit set
  uint32_t* key = reinterpret_cast<uint32_t*>(smem);
  int32_t* perm = reinterpret_cast<int32_t*>(key + kMtN);
  int32_t* vseq = perm + Tm;
  uint32_t* reg = reinterpret_cast<uint32_t*>(vseq + Tm);  // the region
  uint32_t* nxt = reg + W;                                 // the region after this round
  uint8_t* vis = reinterpret_cast<uint8_t*>(nxt + W);
  int pos;  // wave-uniform
  if (a.seed) {
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
  __syncthreads();
  int status = 0, nreg = T;
  if (a.nearby > 0) {
    // 1. i = choice(T)
    int i0 = 0;
    if (T > 1) {
      const uint32_t top = static_cast<uint32_t>(T - 1);
      const uint32_t mask = 0xFFFFFFFFu >> __builtin_clz(top);
      for (;;) {
        if (pos == kMtN) {
          mt_regen<64>(key);
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
    __syncthreads();
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
      __syncthreads();
      int n = 0;
      for (int w = lane; w < W; w += 64) {
        const uint32_t v = nxt[w];
        reg[w] = v;
        n += __popc(v);
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
      __syncthreads();
      if (n == nreg) {
        status |= kResetRegionShort;
        break;
      }
      nreg = n;
    }
  } else {
    for (int t = lane; t < T; t += 64) atomicOr(&reg[t >> 5], 1u << (t & 31));
    __syncthreads();
  }
  uint8_t* region = a.region + (size_t)b * Tm;
  for (int t = lane; t < Tm; t += 64) {
    const uint8_t in = (t < T && ((reg[t >> 5] >> (t & 31)) & 1u)) ? 1 : 0;
    region[t] = in;
    if (a.region_c) a.region_c[(size_t)e * Tm + t] = in;
  }
  if (nreg < R || T < R) {
    // 3'. choice(members, R, replace=False) raises before it draws: the env is not reset
    // (the reset pass skips it; its start row reads -1, its visited row 1)
    status |= kResetRegionSmall;
    for (int k = lane; k < R; k += 64) {
      a.start[(size_t)b * R + k] = -1;
      if (a.start_c) a.start_c[(size_t)e * R + k] = -1;
    }
    for (int t = lane; t < Tm; t += 64) {
      a.visited0[(size_t)b * Tm + t] = 1;
      if (a.visited_c) a.visited_c[(size_t)e * Tm + t] = 1;
    }
  } else {
    // 3. the start targets
    cov_permute(key, pos, perm, vseq, nreg);
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
    __syncthreads();
    for (int k = lane; k < R; k += 64) {
      const int t = vseq[perm[k]];
      a.start[(size_t)b * R + k] = t;
      if (a.start_c) a.start_c[(size_t)e * R + k] = t;
    }
    __syncthreads();
    // 4. the unvisited targets
    cov_permute(key, pos, perm, vseq, T);
    const int kdrop = static_cast<int>(static_cast<double>(T) * a.frac);  // Python's int(T * frac)
    for (int t = lane; t < Tm; t += 64) vis[t] = 1;
    __syncthreads();
    for (int k = lane; k < kdrop; k += 64) vis[perm[k]] = 0;
    __syncthreads();
    for (int t = lane; t < Tm; t += 64) {
      a.visited0[(size_t)b * Tm + t] = vis[t];
      if (a.visited_c) a.visited_c[(size_t)e * Tm + t] = vis[t];
    }
  }
  for (int k = lane; k < kMtN; k += 64) a.mt_key[(size_t)b * kMtN + k] = key[k];
  if (lane == 0) {
    a.mt_pos[b] = pos;
    a.status[b] = status;
    a.nregion[b] = nreg;
    a.envs_ok[e] = (status & kResetRegionSmall) ? -1 : b;
  }
}

}  // namespace

size_t cov_reset_draw_lds_bytes(int Tmax) {
  return (size_t)kMtN * 4 + (size_t)Tmax * 8 + (size_t)((Tmax + 63) / 64) * 16 + (size_t)Tmax;
}

hipError_t launch_cov_reset_draw(const CovResetDrawArgs& a, hipStream_t s) {
  const size_t lds = cov_reset_draw_lds_bytes(a.Tmax);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cov_reset_draw_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cov_reset_draw_kernel, dim3(a.n_sel), dim3(64), lds, s, a);
  return hipGetLastError();
}

}  // namespace gf
