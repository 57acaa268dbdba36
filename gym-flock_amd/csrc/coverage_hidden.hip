// HIP kernels (gfx950) for the hidden-node observation of ExploreEnv-v0 / -v1
// (CoverageARLEnv with hide_nodes=True, n_node_feat=4), batched over envs.
//
// Reference: gym_flock/envs/spatial/coverage.py _get_obs_reward :334-346 (the discovered
// set, the masked node features, the frontier flag, the hidden senders), utils.py
// _nodes_within_radius :27-39, controller :817-821 (the expert's mask).
//
// cov_hidden_kernel, one workgroup per env, runs after the pass that made the env's
// ordinary observation (cov_step_kernel) and reads what that pass left:
//   1. a target is seen when some robot is at distance 0 < sqrt(dx*dx + dy*dy) <= radius
//      (4 * DELTA = 22, whatever the env's res), decided from the squared distance with
//      within_radius' bracket; seen targets join the env's persistent `discovered` bytes.
//      The robots' rows are 1 from the reset on, rows past the last target stay 0. The set
//      is kept as bits in LDS for the passes below;
//   2. over all 4M edge slots, with sender s and receiver q (an index of -1 wraps to node
//      M - 1, as NumPy's does): s undiscovered and q discovered flags q as a frontier node;
//      the slot's sender is kept when both ends are discovered or the slot is one of the
//      last 8R (the action edges), else it becomes -1. Slots between the motion edges and
//      the action edges hold -1 / -1: they flag nothing ((1 - d) * d = 0) and stay -1, so
//      whole 16-byte groups of them are written without being read;
//   3. node rows (M,4): the three ordinary features times the discovered bit, then the
//      frontier flag; the expert's mask visited | !discovered over the targets and its count.
// Every output is rewritten in full, so the arrays never depend on an earlier pass.
#include "coverage_hidden.h"

namespace gf {

namespace {

// cov_hidden_body, the pass over one env: coverage_hidden.h (shared with the explore rollout)
__global__ __launch_bounds__(kHidThreads) void cov_hidden_kernel(CovHiddenArgs a) { cov_hidden_body(a, blockIdx.x); }

// cov_reset_device: the listed envs only (entries < 0 skipped). A kernel of its own, so the
// pass after every step keeps its arguments.
__global__ __launch_bounds__(kHidThreads) void cov_hidden_list_kernel(CovHiddenArgs a, const int32_t* envs) {
  const int b = envs[blockIdx.x];
  if (b < 0) return;
  cov_hidden_body(a, b);
}

// discovered := robots only (reset(), a new graph) for the selected envs
__global__ __launch_bounds__(kHidThreads) void cov_hidden_reset_kernel(CovHiddenArgs a, const int32_t* envs) {
  const int b = envs ? envs[blockIdx.x] : blockIdx.x;
  if (b < 0) return;
  uint8_t* disc = a.discovered + (size_t)b * a.M;
  for (int k = threadIdx.x; k < a.M; k += kHidThreads) disc[k] = k < a.R ? 1 : 0;
}

// unpack_obs (coverage.py:689-741) on the hidden batch: as cov_graphs_kernel, but the edges
// a graph drops are the slots whose hidden sender is -1, wherever they lie, so the kept
// ones are compacted in slot order (one workgroup per env). The reference's offset quirk
// is the same: without mask_all only graph 0 drops anything.
__global__ __launch_bounds__(kHidThreads) void cov_hidden_graphs_kernel(CovHiddenArgs a, const float* edges_in,
                                                                        const int64_t* off, int mask_all,
                                                                        float* edges_out, int32_t* snd_out,
                                                                        int32_t* rcv_out) {
  __shared__ int wsum[kHidThreads / 64 + 1];
  const int b = blockIdx.x;
  const int M = a.M, E = 4 * M;
  const bool keep_all = !mask_all && b > 0;
  const float* edges = edges_in + (size_t)b * E;
  const int32_t* hs = a.hsenders + (size_t)b * E;
  const int32_t* rcv = a.receivers + (size_t)b * E;
  const int32_t shift = b * M;
  int64_t base = off[b];
  const int64_t end = off[b + 1];
  for (int k0 = 0; k0 < E; k0 += kHidThreads) {
    const int k = k0 + threadIdx.x;
    const int s = k < E ? hs[k] : -1;
    const int keep = (k < E && (keep_all || s != -1)) ? 1 : 0;
    int total = 0;
    const int pos = block_exscan<kHidThreads>(keep, wsum, &total);
    const int64_t dst = base + pos;
    if (keep && dst < end) {
      edges_out[dst] = edges[k];
      snd_out[dst] = s + shift;
      rcv_out[dst] = rcv[k] + shift;
    }
    base += total;
  }
}

}  // namespace

size_t cov_hidden_lds_bytes(int R, int M) { return (size_t)R * 16 + (size_t)2 * ((M + 31) / 32) * 4; }

hipError_t launch_cov_hidden(const CovHiddenArgs& a, hipStream_t s) {
  void* args[] = {const_cast<CovHiddenArgs*>(&a)};
  return hipLaunchKernel(reinterpret_cast<const void*>(&cov_hidden_kernel), dim3(a.B), dim3(kHidThreads), args,
                         cov_hidden_lds_bytes(a.R, a.M), s);
}

hipError_t launch_cov_hidden_list(const CovHiddenArgs& a, const int32_t* envs, int n, hipStream_t s) {
  hipLaunchKernelGGL(cov_hidden_list_kernel, dim3(n), dim3(kHidThreads), cov_hidden_lds_bytes(a.R, a.M), s, a, envs);
  return hipGetLastError();
}

hipError_t launch_cov_hidden_reset(const CovHiddenArgs& a, const int32_t* envs, int n, hipStream_t s) {
  hipLaunchKernelGGL(cov_hidden_reset_kernel, dim3(n), dim3(kHidThreads), 0, s, a, envs);
  return hipGetLastError();
}

hipError_t launch_cov_hidden_graphs(const CovHiddenArgs& a, const float* edges_in, const int64_t* off, bool mask_all,
                                    float* edges, int32_t* snd, int32_t* rcv, hipStream_t s) {
  hipLaunchKernelGGL(cov_hidden_graphs_kernel, dim3(a.B), dim3(kHidThreads), 0, s, a, edges_in, off, mask_all ? 1 : 0,
                     edges, snd, rcv);
  return hipGetLastError();
}

}  // namespace gf
