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
#include "coverage_internal.h"

namespace gf {

namespace {

constexpr int kHidThreads = 256;

__device__ __forceinline__ uint32_t hid_bit(const uint32_t* bits, int k) { return (bits[k >> 5] >> (k & 31)) & 1u; }

// The pass over env b (cov_hidden_kernel: the workgroup's index; cov_hidden_list_kernel: an
// entry of a device list)
__device__ __forceinline__ void cov_hidden_body(const CovHiddenArgs& a, const int b) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hid_smem[];
  __shared__ int cnt_s[2];  // kept senders, masked targets
  const int R = a.R, M = a.M, Tm = a.Tmax, E = 4 * M, W = (M + 31) >> 5;
  const int T = min(a.ntg[b], Tm);
  const int tid = threadIdx.x;
  double2* xr_s = reinterpret_cast<double2*>(hid_smem);    // (R) robot positions
  uint32_t* dbits = reinterpret_cast<uint32_t*>(xr_s + R);  // (W) discovered
  uint32_t* fbits = dbits + W;                              // (W) frontier
  const double2* xr = reinterpret_cast<const double2*>(a.xr) + (size_t)b * R;
  const double2* tg = reinterpret_cast<const double2*>(a.tgt) + (size_t)b * Tm;
  uint8_t* disc = a.discovered + (size_t)b * M;
  for (int i = tid; i < R; i += kHidThreads) xr_s[i] = xr[i];
  for (int w = tid; w < W; w += kHidThreads) {
    const int lo = 32 * w;  // the robots' rows are always discovered
    dbits[w] = lo + 32 <= R ? 0xFFFFFFFFu : lo < R ? (1u << (R - lo)) - 1u : 0u;
    fbits[w] = 0u;
  }
  if (tid < 2) cnt_s[tid] = 0;
  __syncthreads();
  // 1. discovery
  const double r = a.radius, rr = r * r;
  const double r2lo = rr * (1.0 - 0x1p-50), r2hi = rr * (1.0 + 0x1p-50);
  for (int t = tid; t < T; t += kHidThreads) {
    bool d = disc[R + t] != 0;
    if (!d) {
      const double2 p = tg[t];
      for (int i = 0; i < R && !d; ++i) {
        const double dx = xr_s[i].x - p.x, dy = xr_s[i].y - p.y;
        d = within_radius(dx * dx + dy * dy, r, r2lo, r2hi);
      }
      if (d) disc[R + t] = 1;
    }
    if (d) atomicOr(&dbits[(R + t) >> 5], 1u << ((R + t) & 31));
  }
  __syncthreads();
  // 2. frontier flags and hidden senders, 4 slots per thread and pass
  const int nm = a.n_motion[b], tail0 = E - 8 * R;
  const int4* snd4 = reinterpret_cast<const int4*>(a.senders + (size_t)b * E);
  const int4* rcv4 = reinterpret_cast<const int4*>(a.receivers + (size_t)b * E);
  int4* hs4 = reinterpret_cast<int4*>(a.hsenders + (size_t)b * E);
  int kept = 0;
  for (int g = tid; g < M; g += kHidThreads) {
    const int k0 = 4 * g;
    if (k0 >= nm && k0 + 4 <= tail0) {  // unused slots only
      hs4[g] = make_int4(-1, -1, -1, -1);
      continue;
    }
    const int4 s4 = snd4[g], q4 = rcv4[g];
    const int sv[4] = {s4.x, s4.y, s4.z, s4.w}, qv[4] = {q4.x, q4.y, q4.z, q4.w};
    int o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int s = sv[j] < 0 ? sv[j] + M : sv[j], q = qv[j] < 0 ? qv[j] + M : qv[j];
      const bool ok = static_cast<unsigned>(s) < static_cast<unsigned>(M) && static_cast<unsigned>(q) < static_cast<unsigned>(M);
      const uint32_t ds = ok ? hid_bit(dbits, s) : 0u, dq = ok ? hid_bit(dbits, q) : 0u;
      if (ok && !ds && dq) atomicOr(&fbits[q >> 5], 1u << (q & 31));
      o[j] = ((ds & dq) || k0 + j >= tail0) ? sv[j] : -1;
      kept += o[j] != -1 ? 1 : 0;
    }
    hs4[g] = make_int4(o[0], o[1], o[2], o[3]);
  }
  // the expert's mask: visited or undiscovered targets (slots past the last target stay 1)
  const uint8_t* vis = a.visited + (size_t)b * Tm;
  uint8_t* gm = a.gmask + (size_t)b * Tm;
  int masked = 0;
  for (int t = tid; t < Tm; t += kHidThreads) {
    const uint8_t m = t < T ? ((vis[t] || !hid_bit(dbits, R + t)) ? 1 : 0) : 1;
    gm[t] = m;
    masked += (t < T && m) ? 1 : 0;
  }
  atomicAdd(&cnt_s[0], kept);
  atomicAdd(&cnt_s[1], masked);
  __syncthreads();
  // 3. node rows
  const float* nodes = a.nodes + (size_t)b * M * 3;
  float4* hn = reinterpret_cast<float4*>(a.hnodes) + (size_t)b * M;
  for (int k = tid; k < M; k += kHidThreads) {
    const bool d = hid_bit(dbits, k);
    hn[k] = make_float4(d ? nodes[3 * k] : 0.0f, d ? nodes[3 * k + 1] : 0.0f, d ? nodes[3 * k + 2] : 0.0f,
                        hid_bit(fbits, k) ? 1.0f : 0.0f);
  }
  if (tid == 0) {
    a.nkeep[b] = cnt_s[0];
    a.ngmask[b] = cnt_s[1];
  }
}

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
