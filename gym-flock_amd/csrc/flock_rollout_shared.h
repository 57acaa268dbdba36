// What the closed-loop rollout kernels of FlockingRelative share (flock_rollout.hip, the
// expert's; flock_policy_rollout.hip, the DAgger loop's): the workgroup's size and the
// deterministic sums over a row's four threads, a wave and the workgroup's wave slots.
#pragma once
#include "flock_internal.h"

namespace gf {

namespace {

constexpr int kRolloutThreads = 1024;
constexpr int kRolloutWaves = kRolloutThreads / 64;

// v of the lane a DPP control selects (quad_perm [1,0,3,2] 0xB1, [2,3,0,1] 0x4E,
// row_half_mirror 0x141, row_mirror 0x140): in a butterfly whose half groups already
// agree, these give the partial sums a shfl_xor by 1, 2, 4, 8 would, without its LDS trip
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

// butterfly sum over aligned groups of G lanes: every lane ends with the same bits
template <int G>
__device__ __forceinline__ double group_sum(double v) {
  if constexpr (G > 1) v += dpp_f64<0xB1>(v);
  if constexpr (G > 2) v += dpp_f64<0x4E>(v);
  if constexpr (G > 4) v += dpp_f64<0x141>(v);
  if constexpr (G > 8) v += dpp_f64<0x140>(v);
#pragma unroll
  for (int o = 16; o < G; o <<= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_sum64(double v) { return group_sum<64>(v); }
__device__ __forceinline__ double row_sum4(double v) { return group_sum<4>(v); }

// The 16 wave slots (x, y) of `red` summed in a fixed pairwise tree, by a whole wave: lane l
// takes slot l % 16 and a butterfly over 16 lanes leaves ((s0 + s1) + (s2 + s3)) + ... in
// every lane.
__device__ __forceinline__ double2 slot_sum(const double2* red, int lane) {
  const double2 v = red[lane & (kRolloutWaves - 1)];
  return double2{group_sum<kRolloutWaves>(v.x), group_sum<kRolloutWaves>(v.y)};
}

}  // namespace

}  // namespace gf
