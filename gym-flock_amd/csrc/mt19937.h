// numpy's legacy RandomState generator on the device (MT19937, the published algorithm of
// Matsumoto & Nishimura), shared by the Coverage kernels (np_random, the map streams) and
// the flocking reset (flock_reset.hip). A stream is RandomState.get_state()'s key words
// and position.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gf {

constexpr int kMtN = 624, kMtM = 397;
__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  return y ^ (y >> 18);
}
__device__ __forceinline__ uint32_t mt_mix(uint32_t cur, uint32_t next, uint32_t far) {
  const uint32_t y = (cur & 0x80000000u) | (next & 0x7fffffffu);
  return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}
// How the threads that share a key in LDS order their accesses to it. WgSync: the workgroup's
// barrier (every thread of the workgroup takes part). WaveSync: one wave working alone while
// the workgroup's other waves wait at a later barrier (cov_rollout_kernel's reset draws): a
// wave's LDS instructions execute in issue order, so only the compiler must keep them in order.
struct WgSync {
  __device__ __forceinline__ void operator()() const { __syncthreads(); }
};
struct WaveSync {
  __device__ __forceinline__ void operator()() const {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
  }
};
// The key's regeneration (after 624 outputs) by the whole workgroup on a key in LDS. Word i
// mixes words i, i+1 and i+397 (mod 624, the wrapped ones already regenerated), so three
// passes of at most 227 independent words each, then word 623: [0,227) reads only old
// words, [227,454) reads the first pass's results, [454,623) the second's. Ends with a
// barrier. Every thread of the workgroup calls it (Sync = WaveSync: every lane of the one
// wave, NT = 64). tid: the caller's index among the NT threads that share the work; a
// thread beyond them passes kMtN and only keeps the barriers.
template <int NT, class Sync = WgSync>
__device__ __forceinline__ void mt_regen(uint32_t* k, const int tid = static_cast<int>(threadIdx.x)) {
  const Sync sync;
  constexpr int P = kMtN - kMtM;  // 227
  constexpr int S = (P + NT - 1) / NT;
  auto pass = [&](int lo, int hi) {
    uint32_t v[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int i = lo + tid + s * NT;
      if (i < hi) v[s] = mt_mix(k[i], k[i + 1], k[i < P ? i + kMtM : i - P]);
    }
    sync();
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int i = lo + tid + s * NT;
      if (i < hi) k[i] = v[s];
    }
    sync();
  };
  pass(0, P);
  pass(P, 2 * P);
  pass(2 * P, kMtN - 1);
  if (tid == 0) k[kMtN - 1] = mt_mix(k[kMtN - 1], k[0], k[kMtM - 1]);
  sync();
}

}  // namespace gf
