// cov_expert_rollout (gfx950): recorded greedy expert rollouts of the plain Coverage envs
// across episode ends in one launch.
//
// One workgroup per env, n_steps iterations, the launch shape of cov_step_multi_kernel. An
// iteration of env b is
//   1. the fused greedy expert step with the device fallback draws (cov_step_body<NT, true>,
//      coverage_step.h), which writes the reward and done flag at [it][b];
//   2. this step's actions and needs-random flags into the records at [it][b][:];
//   3. AR (auto-reset), when the step has just set done[b] (the flag is read after a barrier,
//      so the decision is uniform over the workgroup): the reference's reset() on the
//      unchanged map (coverage.py:398-424, graph_changed == False), which is what
//      cov_reset_device does without new maps:
//        - wave 0 runs cov_reset_device's draws for the env (cov_reset_draw_body,
//          coverage_reset_draw.h) from the env's stream where the step left it, in LDS of its
//          own, and leaves the stream in mt_key / mt_pos; the other waves wait at the barrier
//          behind it (the wave orders its own LDS accesses: WaveSync, mt19937.h);
//        - a region with fewer nodes than robots: the env keeps its state and goes on
//          stepping, its stream advanced by the scalar draw;
//        - else the workgroup runs cov_reset_kernel's pass (cov_reset_pass) and then the
//          observation pass that finish_reset launches as cov_step_list_kernel
//          (cov_step_body<NT, false> without actions or greedy lists);
//   4. on a recorded iteration the env's flat row from what the workgroup has just written
//      (the row after the reset where one has just happened).
// Everything an iteration reads of earlier global writes (the robots' nodes, the tail's
// offers, the visited flags, the env's words, the start and visited rows, the key) was written
// by this workgroup, and the barriers between the passes order it (as in
// cov_step_multi_kernel). AR is a template parameter: the launch without auto-reset carries
// none of the reset's code or LDS.
#include "coverage_reset_draw.h"
#include "coverage_step.h"

namespace gf {

namespace {

template <int NT, bool AR>
__global__ __launch_bounds__(NT) void cov_rollout_kernel(CovArgsR p0) {
  static_assert(NT == kCovThreads, "the reset pass strides by kCovThreads");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  [[maybe_unused]] __shared__ int count_s;   // the reset pass's visited count
  [[maybe_unused]] __shared__ int status_s;  // the draws' status, from wave 0 to the workgroup
  // The arguments are read from the kernel argument segment anew at every phase of every
  // iteration (the pointer passes through an empty asm): kept live across the loop or across
  // the reset branch, the step's fifty-odd pointers overflow the scalar registers and spill
  // into vector ones (cov_step_multi_kernel's 221 VGPRs against the one-step kernel's 79).
  using KArgs = const __attribute__((address_space(4))) CovArgsR;
  KArgs* kp = (KArgs*)__builtin_amdgcn_kernarg_segment_ptr();  // the one argument, at offset 0
  auto args = [&]() -> const CovArgsR& {
    asm volatile("" : "+s"(kp));
    return *(const CovArgsR*)kp;
  };
  const int tid = threadIdx.x;
  [[maybe_unused]] const int b0 = AR ? p0.a.env0 + static_cast<int>(blockIdx.x) : 0;
  const int n = p0.n_steps > 1 ? p0.n_steps : 1;
  [[maybe_unused]] int nres = 0, stat = 0;  // thread 0's are written out
  for (int it = 0; it < n; ++it) {
    const CovArgsR& p = args();
    // the env, in the form with which the instantiation reserves no private segment: the other
    // form makes the compiler reserve 36 bytes per lane (save slots of the vector registers
    // that hold spilled scalar ones) which no instruction ever touches
    const int b = AR ? b0 : p.a.env0 + blockIdx.x;
    cov_step_body<NT, true>(p.a, b, it, p.reward_k, p.done_k);
    __syncthreads();  // the step's flags, actions and observation, written by other threads
    bool ended;
    {
      const CovArgs& a = p.a;
      const int R = a.R;
      const size_t row = ((size_t)it * a.B + b) * R;
      if (p.act_k)
        for (int i = tid; i < R; i += NT) p.act_k[row + i] = a.gactions[(size_t)b * R + i];
      if (p.nrand_k)
        for (int i = tid; i < R; i += NT) p.nrand_k[row + i] = a.needs_random[(size_t)b * R + i];
      ended = AR && a.done[b];  // uniform: one byte, read by every thread after the barrier
    }
    if constexpr (AR) {
      if (ended) {
        const CovArgsR& pd = args();
        if (tid < 64) {
          const int st = cov_reset_draw_body<true, WaveSync>(pd.d, 0, b, smem + pd.draw_off);
          if (tid == 0) status_s = st;
        }
        __syncthreads();  // the start row, the visited row, the stream and the status
        const int st = status_s;
        stat |= st;
        if (!(st & kResetRegionSmall)) {
          ++nres;
          {
            const CovArgsR& pr = args();
            cov_reset_pass(pr.a, b, pr.d.start, pr.d.visited0, &count_s);
          }
          __syncthreads();  // the robots, the flags and the env's words before the observation pass
          {
            CovArgs o = args().a;  // finish_reset's arguments: no actions, no greedy lists, no streams
            o.actions = nullptr;
            o.glist = nullptr;
            o.glen = nullptr;
            o.gcost = nullptr;
            o.gprev = nullptr;
            o.gactions = nullptr;
            o.needs_random = nullptr;
            o.mt_key = nullptr;
            o.mt_pos = nullptr;
            cov_step_body<NT, false>(o, b, 0, nullptr, nullptr);
          }
          __syncthreads();
        }
      }
    }
    if (p.flat_k && (it + 1) % p.record_every == 0) {
      const CovArgs& a = p.a;
      const int M = a.M;
      const size_t L = (size_t)15 * M + 1;
      float* out = p.flat_k + ((size_t)((it + 1) / p.record_every - 1) * a.B + b) * L;
      const float* nodes = a.nodes + (size_t)b * M * 3;
      const float* edges = a.edges + (size_t)b * 4 * M;
      const int32_t* snd = a.senders + (size_t)b * 4 * M;
      const int32_t* rcv = a.receivers + (size_t)b * 4 * M;
      for (size_t k = tid; k < L; k += NT)
        out[k] = cov_flat_value<float>(k, (size_t)M, (size_t)3 * M, nodes, edges, snd, rcv, a.obs_step + b);
      __syncthreads();  // the row is read before the next step rewrites its sources
    }
  }
  if constexpr (AR) {
    if (tid == 0) {
      if (p0.n_resets) p0.n_resets[b0] = nres;
      if (p0.status) p0.status[b0] = stat;
    }
  }
}

}  // namespace

size_t cov_rollout_lds_layout(int R, int M, bool auto_reset, int* draw_off) {
  const size_t off = (cov_step_lds_bytes(R, M) + 15) & ~(size_t)15;
  if (draw_off) *draw_off = (int)off;
  return auto_reset ? off + cov_reset_draw_lds_bytes(M - R) : cov_step_lds_bytes(R, M);
}

hipError_t launch_cov_rollout(const CovArgsR& x, hipStream_t s) {
  CovArgsR p = x;
  const size_t lds = cov_rollout_lds_layout(p.a.R, p.a.M, p.auto_reset != 0, &p.draw_off);
  if (lds > kCovRolloutLdsMax) return hipErrorInvalidValue;
  void* args[] = {&p};
  const void* k = p.auto_reset ? reinterpret_cast<const void*>(&cov_rollout_kernel<kCovThreads, true>)
                               : reinterpret_cast<const void*>(&cov_rollout_kernel<kCovThreads, false>);
  return hipLaunchKernel(k, dim3(p.a.B), dim3(kCovThreads), args, lds, s);
}

}  // namespace gf
