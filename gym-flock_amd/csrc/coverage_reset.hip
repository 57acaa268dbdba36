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
#include "coverage_reset_draw.h"

namespace gf {

namespace {

__global__ __launch_bounds__(64) void cov_reset_draw_kernel(CovResetDrawArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int e = blockIdx.x;
  if (e >= a.n_sel) return;
  cov_reset_draw_body<false, WgSync>(a, e, a.envs[e], smem);  // coverage_reset_draw.h
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
