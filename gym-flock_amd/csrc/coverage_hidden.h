// The hidden-node pass of one env (coverage_hidden.hip has the account of what it computes),
// one body for the pass after every observation (cov_hidden_kernel) and for the fused
// explore rollout (cov_explore_multi_kernel, coverage_kernels.hip), so both run the same code.
#pragma once
#include "coverage_internal.h"

namespace gf {

constexpr int kHidThreads = 256;

__device__ __forceinline__ uint32_t hid_bit(const uint32_t* bits, int k) { return (bits[k >> 5] >> (k & 31)) & 1u; }

// word w of the discovered bits with the robots' rows only (they are always discovered)
__device__ __forceinline__ uint32_t hid_robot_word(int w, int R) {
  const int lo = 32 * w;
  return lo + 32 <= R ? 0xFFFFFFFFu : lo < R ? (1u << (R - lo)) - 1u : 0u;
}

// The pass over env b (cov_hidden_kernel: the workgroup's index; cov_hidden_list_kernel: an
// entry of a device list).
// KEPT (the rollout): the caller keeps the pass's LDS for a whole launch at `lds`, laid out
// as below and followed by the two counters: the robots' positions and the WHOLE discovered
// set as bits are current on entry (a barrier has passed since they were written), so what
// is already discovered is read from the bits, not from the persistent bytes; tg_in: the
// env's targets (in LDS); with full == false (uniform over the workgroup) the pass ends
// after the discovery, else it goes on as ever, rewriting every output.
template <bool KEPT = false>
__device__ __forceinline__ void cov_hidden_body(const CovHiddenArgs& a, const int b,
                                                [[maybe_unused]] unsigned char* lds = nullptr,
                                                [[maybe_unused]] const double2* tg_in = nullptr,
                                                [[maybe_unused]] const bool full = true) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hid_smem_own[];
  __shared__ int cnt_own[2];  // kept senders, masked targets
  const int R = a.R, M = a.M, Tm = a.Tmax, E = 4 * M, W = (M + 31) >> 5;
  const int T = min(a.ntg[b], Tm);
  const int tid = threadIdx.x;
  unsigned char* hid_smem = KEPT ? lds : hid_smem_own;
  double2* xr_s = reinterpret_cast<double2*>(hid_smem);    // (R) robot positions
  uint32_t* dbits = reinterpret_cast<uint32_t*>(xr_s + R);  // (W) discovered
  uint32_t* fbits = dbits + W;                              // (W) frontier
  int* cnt_s = KEPT ? reinterpret_cast<int*>(fbits + W) : cnt_own;
  const double2* xr = reinterpret_cast<const double2*>(a.xr) + (size_t)b * R;
  const double2* tg = KEPT ? tg_in : reinterpret_cast<const double2*>(a.tgt) + (size_t)b * Tm;
  uint8_t* disc = a.discovered + (size_t)b * M;
  if constexpr (!KEPT) {
    for (int i = tid; i < R; i += kHidThreads) xr_s[i] = xr[i];
    for (int w = tid; w < W; w += kHidThreads) {
      dbits[w] = hid_robot_word(w, R);
      fbits[w] = 0u;
    }
    if (tid < 2) cnt_s[tid] = 0;
    __syncthreads();
  }
  // 1. discovery
  const double r = a.radius, rr = r * r;
  const double r2lo = rr * (1.0 - 0x1p-50), r2hi = rr * (1.0 + 0x1p-50);
  for (int t = tid; t < T; t += kHidThreads) {
    bool d = KEPT ? hid_bit(dbits, R + t) != 0u : disc[R + t] != 0;
    [[maybe_unused]] const bool known = d;
    if (!d) {
      const double2 p = tg[t];
      for (int i = 0; i < R && !d; ++i) {
        const double dx = xr_s[i].x - p.x, dy = xr_s[i].y - p.y;
        d = within_radius(dx * dx + dy * dy, r, r2lo, r2hi);
      }
      if (d) disc[R + t] = 1;
    }
    if (KEPT ? (d && !known) : d) atomicOr(&dbits[(R + t) >> 5], 1u << ((R + t) & 31));
  }
  if constexpr (KEPT) {
    if (!full) return;
    for (int w = tid; w < W; w += kHidThreads) fbits[w] = 0u;
    if (tid < 2) cnt_s[tid] = 0;
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

}  // namespace gf
