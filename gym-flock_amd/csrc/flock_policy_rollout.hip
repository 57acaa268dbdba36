// DAgger rollouts of FlockingRelative in one launch (fe_step_policy): the closed loop of
// flock_rollout.hip in which every step's action is the expert's (controller()) or a
// learner's, a small network shared by all agents that reads delayed aggregation features
// (Tolstaya et al., CoRL 2020), chosen per step and env; the expert's action of every state
// the loop reaches is the label. Built with -ffp-contract=off.
//
// The layout is the expert rollout's: one workgroup per env of N <= kRolloutMaxN agents, four
// threads per agent, thread q of row i over the columns [q * CB, (q + 1) * CB); the float64
// state in LDS by the step's parity; pass 1 marks the candidates, pass 2 runs over them;
// the same sums in the same order, ONE workgroup barrier per step. See flock_rollout.hip for
// all of that; what follows is what this kernel adds.
//
// Aggregation. z_t[i, 0, :] is the step's float32 state_values; for k >= 1,
//   z_t[i, k, :] = float32((sum over j adjacent to i in state t of double(z_{t-1}[j, k-1, :])) / d_i),
// d_i = max(deg_i, 1) with mean pooling, else 1: a product of the dense network with the
// previous state's taps, formed from the row's adjacency bits (pass 3: a thread adds the
// taps of its adjacent columns in ascending j, the row's four threads are combined by the
// features' butterfly, so all four end with the same bits). The dense network is never
// written. Taps 0 .. K-2 of the previous state sit in LDS as float32, by the step's parity:
// step t reads buffer t & 1 and the row's owner writes the new state's into the other, which
// the next step's barrier publishes.
//
// Policy. The network's weights are in LDS (PolicyNet's layout). All four threads of a row
// hold the row's 6K inputs; a hidden layer's outputs are split over them, Pw = width / 4
// consecutive outputs each, every output its own float32 sum: bias first, then w[o, i] * x[i]
// for i ascending, product and sum rounded separately. A layer's inputs that live in the
// other threads' registers come by a quad broadcast (DPP) in that same order. The two
// outputs are summed by the row's threads 0 and 1. Nothing here depends on N or the batch.
// Register arrays are indexed by constants only: the loops over inputs and outputs are
// unrolled to the largest network, with wave-uniform guards on the real widths.
#include "flock_dynamics.h"
#include "flock_internal.h"
#include "flock_rollout_shared.h"

namespace gf {

namespace {

constexpr int kZ = 6 * kPolicyMaxTaps;          // inputs of the largest network
constexpr int kHid = kPolicyMaxWidth / 4;       // a thread's outputs of the widest layer
constexpr size_t kLdsState = 2 * sizeof(St) * kRolloutMaxN;
constexpr size_t kLdsRed = 2 * sizeof(double2) * kRolloutWaves;
constexpr size_t kLdsFixed = kLdsState + 2 * kLdsRed;

// lane S of every quad
template <int S>
__device__ __forceinline__ float quad_bcast(float v) {
  constexpr int ctrl = S | (S << 2) | (S << 4) | (S << 6);
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xF, 0xF, false));
}

// acc[.] += w[., i] * xi for this thread's outputs: P4 float4s of row i of the layer
__device__ __forceinline__ void hidden_add(const float* w, int i, int stride, int qoff, int P4, float xi,
                                           float (&acc)[kHid]) {
  const float4* wr = reinterpret_cast<const float4*>(w + i * stride + qoff);
#pragma unroll
  for (int g = 0; g < kHid / 4; ++g) {
    if (g < P4) {
      const float4 ww = wr[g];
      acc[4 * g + 0] = acc[4 * g + 0] + ww.x * xi;
      acc[4 * g + 1] = acc[4 * g + 1] + ww.y * xi;
      acc[4 * g + 2] = acc[4 * g + 2] + ww.z * xi;
      acc[4 * g + 3] = acc[4 * g + 3] + ww.w * xi;
    }
  }
}

template <int S>
__device__ __forceinline__ void hidden_from_lane(const float* w, int Pin, int stride, int qoff, int P4,
                                                 const float (&hin)[kHid], float (&acc)[kHid]) {
#pragma unroll
  for (int m = 0; m < kHid; ++m)
    if (m < Pin) hidden_add(w, S * Pin + m, stride, qoff, P4, quad_bcast<S>(hin[m]), acc);
}

// One hidden layer with ReLU. FROM_Z: the inputs are z (the same in the row's four threads);
// else input i = s * Pin + m is hin[m] of the row's thread s (Pin = n_in / 4).
template <bool FROM_Z>
__device__ __forceinline__ void hidden_layer(const float* w, const float* bias, int n_in, int w_out, int q,
                                             const float (&z)[kZ], const float (&hin)[kHid], float (&out)[kHid]) {
  const int Pw = w_out >> 2, P4 = (Pw + 3) >> 2, PS = P4 << 2, stride = PS << 2, qoff = q * PS;
  float acc[kHid];
  const float4* bq = reinterpret_cast<const float4*>(bias + qoff);
#pragma unroll
  for (int g = 0; g < kHid / 4; ++g) {
    float4 v{0.f, 0.f, 0.f, 0.f};
    if (g < P4) v = bq[g];
    acc[4 * g + 0] = v.x;
    acc[4 * g + 1] = v.y;
    acc[4 * g + 2] = v.z;
    acc[4 * g + 3] = v.w;
  }
  if constexpr (FROM_Z) {
#pragma unroll
    for (int i = 0; i < kZ; ++i)
      if (i < n_in) hidden_add(w, i, stride, qoff, P4, z[i], acc);
  } else {
    const int Pin = n_in >> 2;
    hidden_from_lane<0>(w, Pin, stride, qoff, P4, hin, acc);
    hidden_from_lane<1>(w, Pin, stride, qoff, P4, hin, acc);
    hidden_from_lane<2>(w, Pin, stride, qoff, P4, hin, acc);
    hidden_from_lane<3>(w, Pin, stride, qoff, P4, hin, acc);
  }
#pragma unroll
  for (int m = 0; m < kHid; ++m) out[m] = acc[m] > 0.f ? acc[m] : 0.f;  // ReLU
}

template <int S>
__device__ __forceinline__ float last_from_lane(const float* w, int Pin, int q, const float (&hin)[kHid], float acc) {
#pragma unroll
  for (int m = 0; m < kHid; ++m)
    if (m < Pin) acc = acc + w[(S * Pin + m) * 4 + q] * quad_bcast<S>(hin[m]);
  return acc;
}

// The last layer: output o summed by the row's thread o (threads 2 and 3 sum zeros); both
// outputs, clipped, in every thread of the row.
template <bool FROM_Z>
__device__ __forceinline__ float2 last_layer(const float* w, const float* bias, int n_in, int q, float clip,
                                             const float (&z)[kZ], const float (&hin)[kHid]) {
  float acc = bias[q];
  if constexpr (FROM_Z) {
#pragma unroll
    for (int i = 0; i < kZ; ++i)
      if (i < n_in) acc = acc + w[i * 4 + q] * z[i];
  } else {
    const int Pin = n_in >> 2;
    acc = last_from_lane<0>(w, Pin, q, hin, acc);
    acc = last_from_lane<1>(w, Pin, q, hin, acc);
    acc = last_from_lane<2>(w, Pin, q, hin, acc);
    acc = last_from_lane<3>(w, Pin, q, hin, acc);
  }
  if (clip > 0.f) acc = clip_sym(acc, clip);
  return float2{quad_bcast<0>(acc), quad_bcast<1>(acc)};
}

// Run by whole waves (the quad broadcasts read every lane): rows past N - 1 compute on zeros.
__device__ __forceinline__ float2 policy_mlp(const PolicyNet& n, const float* wl, int q, const float (&z)[kZ]) {
  float h0[kHid], h1[kHid];
#pragma unroll
  for (int m = 0; m < kHid; ++m) h0[m] = 0.f;
  const int L = n.n_layers;
  if (L == 1) return last_layer<true>(wl + n.off_w[0], wl + n.off_b[0], n.width[0], q, n.clip, z, h0);
  hidden_layer<true>(wl + n.off_w[0], wl + n.off_b[0], n.width[0], n.width[1], q, z, h0, h1);
  if (L == 2) return last_layer<false>(wl + n.off_w[1], wl + n.off_b[1], n.width[1], q, n.clip, z, h1);
  hidden_layer<false>(wl + n.off_w[1], wl + n.off_b[1], n.width[1], n.width[2], q, z, h1, h0);
  return last_layer<false>(wl + n.off_w[2], wl + n.off_b[2], n.width[2], q, n.clip, z, h0);
}

template <int CB>
__global__ __launch_bounds__(CB * 16) void flock_policy_rollout_kernel(PolicyRolloutArgs pa) {
  const RolloutArgs& p = pa.r;
  const StepArgs& a = p.s;
  const PolicyNet& net = pa.net;
  // policy_rollout_lds_bytes: the state by parity; per wave the (vx, vy) sums and the squared
  // deviations by parity; the network; the previous state's taps 0 .. K-2 by parity
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  St(*st)[kRolloutMaxN] = reinterpret_cast<St(*)[kRolloutMaxN]>(lds);
  double2(*red1)[kRolloutWaves] = reinterpret_cast<double2(*)[kRolloutWaves]>(lds + kLdsState);
  double2(*red2)[kRolloutWaves] = reinterpret_cast<double2(*)[kRolloutWaves]>(lds + kLdsState + kLdsRed);
  float* wl = reinterpret_cast<float*>(lds + kLdsFixed);
  float* tapbuf = wl + ((net.n_floats + 3) & ~3);

  const int N = a.N, B = a.B, b = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int Wn = (N + 63) >> 6;
  const int row = tid >> 2, q = tid & 3;
  const bool inrow = row < N;
  const bool owner = q == 0 && inrow;
  const int jb = q * CB;
  const size_t g = (size_t)b * N + row;
  const double Nd = static_cast<double>(N);
  const double tmax = a.cr > a.cr2 ? a.cr : a.cr2;
  const int K = net.n_taps;
  const int TS = (K - 1) * 6;   // floats of a row's taps in LDS, and of the handle's
  if (tid < 2 * kRolloutWaves) {
    red1[tid >> 4][tid & 15] = double2{0.0, 0.0};
    red2[tid >> 4][tid & 15] = double2{0.0, 0.0};
  }
  for (int i = tid; i < net.n_floats; i += blockDim.x) wl[i] = net.image[i];

  St me{0.0, 0.0, 0.0, 0.0};
  double2 u{0.0, 0.0};
  if (owner) {
    const double2* xp = reinterpret_cast<const double2*>(a.x_in) + 2 * g;
    const double2 pp = xp[0], vv = xp[1];
    me = St{pp.x, pp.y, vv.x, vv.y};
    u = reinterpret_cast<const double2*>(a.u)[g];
  }
  // the aggregation of the state before the first step: tap 0 is its state_values
  float z[kZ];
#pragma unroll
  for (int i = 0; i < kZ; ++i) z[i] = 0.f;
  if (inrow) {
#pragma unroll
    for (int f = 0; f < 6; ++f) z[f] = a.state_values[g * 6 + f];
#pragma unroll
    for (int k = 1; k < kPolicyMaxTaps; ++k)
      if (k < K) {
#pragma unroll
        for (int f = 0; f < 6; ++f) z[6 * k + f] = pa.taps[g * TS + (k - 1) * 6 + f];
      }
  }
  if (owner) {
    float* tw = tapbuf + (size_t)row * TS;
#pragma unroll
    for (int k = 0; k < kPolicyMaxTaps - 1; ++k)
      if (k < K - 1) {
#pragma unroll
        for (int f = 0; f < 6; ++f) tw[6 * k + f] = z[6 * k + f];
      }
  }
  __syncthreads();  // the network, the wave slots (the taps wait for the first step's barrier)
  float2 pol;

  auto emit_reward = [&](int t) {
    const double2 Q = slot_sum(red2[t & 1], lane);
    if (tid == 0) {
      const double rw = -1.0 * (Q.x / Nd + Q.y / Nd);
      if (p.rec_rewards) p.rec_rewards[(size_t)t * B + b] = rw;
      if (t == p.n_steps - 1 && a.reward) a.reward[b] = rw;
    }
  };

  int ue = pa.mask ? pa.mask[b] : pa.mask_const;
  bool rec_prev = false;
  size_t gr_prev = 0;
  for (int t = 0;; ++t) {
    // the learner's action of the current state (one site: the code is long); the record of
    // the step before is this state's
    pol = policy_mlp(net, wl, q, z);
    if (owner && rec_prev && pa.rec_policy) reinterpret_cast<float2*>(pa.rec_policy)[gr_prev] = pol;
    if (t == p.n_steps) break;
    St* cur = st[t & 1];
    const float* tprev = tapbuf + (size_t)(t & 1) * N * TS;
    float* tnext = tapbuf + (size_t)((t + 1) & 1) * N * TS;
    // the next step's choice, loaded a step ahead: the one global read of a step
    int ue_next = ue;
    if (pa.mask && t + 1 < p.n_steps) ue_next = pa.mask[(size_t)(t + 1) * B + b];
    if (tid == 0 && pa.rec_used) pa.rec_used[(size_t)t * B + b] = ue ? 1 : 0;
    if (owner) {
      const double2 ap = ue ? u : double2{static_cast<double>(pol.x), static_cast<double>(pol.y)};
      if (pa.rec_applied) reinterpret_cast<double2*>(pa.rec_applied)[((size_t)t * B + b) * N + row] = ap;
      const double2 pp{me.px, me.py}, vv{me.vx, me.vy};
      me = integrate_plain<true>(a, pp, vv, ap);
      cur[row] = me;
    }
    {
      const double sx = wave_sum64(owner ? me.vx : 0.0), sy = wave_sum64(owner ? me.vy : 0.0);
      if (lane == 0) red1[t & 1][wid] = double2{sx, sy};
    }
    __syncthreads();  // the step's state and velocity sums, the previous state's taps
    if (wid == 0 && t > 0) emit_reward(t - 1);

    const double2 Sv = slot_sum(red1[t & 1], lane);
    {
      const double ex = me.vx - Sv.x / Nd, ey = me.vy - Sv.y / Nd;
      const double qx = wave_sum64(owner ? ex * ex : 0.0), qy = wave_sum64(owner ? ey * ey : 0.0);
      if (lane == 0) red2[t & 1][wid] = double2{qx, qy};
    }

    // pass 1: the candidates among this thread's CB columns
    St r{0.0, 0.0, 0.0, 0.0};
    uint64_t mc = 0;
    if (inrow) {
      r = cur[row];
#pragma unroll 16
      for (int c = 0; c < CB; ++c) {
        const double2 pj = *reinterpret_cast<const double2*>(&cur[(jb + c) & (kRolloutMaxN - 1)]);
        const double dx = r.px - pj.x, dy = r.py - pj.y;
        const double r2 = dx * dx + dy * dy;
        mc |= !(r2 > tmax) ? (1ull << c) : 0ull;
      }
      const int nv = N - jb;
      mc &= nv >= 64 ? ~0ull : (nv > 0 ? (1ull << nv) - 1ull : 0ull);
      const int dg = row - jb;
      if (dg >= 0 && dg < CB) mc &= ~(1ull << dg);
    }

    // pass 2: compute_helpers and controller over the candidates
    double f0 = 0, f1 = 0, f2 = 0, f3 = 0, f4 = 0, f5 = 0, gx = 0, gy = 0;
    uint64_t ma = 0;
    while (mc) {
      const int c = __builtin_ctzll(mc);
      mc &= mc - 1;
      const St o = cur[jb + c];
      const double dx = r.px - o.px, dy = r.py - o.py;
      const double r2 = dx * dx + dy * dy;
      const bool isadj = r2 < a.cr2;
      const bool far = r2 > a.cr;
      const double ir = 1.0 / r2, irr = ir * ir;
      const double q1x = dx * irr, q2x = dx * ir;
      const double q1y = dy * irr, q2y = dy * ir;
      if (isadj) {
        ma |= 1ull << c;
        f0 += r.vx - o.vx;
        f1 += q1x;
        f2 += q2x;
        f3 += r.vy - o.vy;
        f4 += q1y;
        f5 += q2y;
      }
      if (!far && (a.centralized || isadj)) {
        gx += (-2.0 * q1x) + (2.0 * q2x);
        gy += (-2.0 * q1y) + (2.0 * q2y);
      }
    }
    f0 = row_sum4(f0);
    f1 = row_sum4(f1);
    f2 = row_sum4(f2);
    f3 = row_sum4(f3);
    f4 = row_sum4(f4);
    f5 = row_sum4(f5);
    gx = row_sum4(gx);
    gy = row_sum4(gy);
    int deg = __popcll(ma);
    deg += __shfl_xor(deg, 1);
    deg += __shfl_xor(deg, 2);
    uint64_t word = ma << ((q * CB) & 63);
    int wq = 0;
    bool hasw = false;
    if constexpr (CB == 16) {
      word |= __shfl_xor(word, 1);
      word |= __shfl_xor(word, 2);
      hasw = q == 0;
    } else if constexpr (CB == 32) {
      word |= __shfl_xor(word, 1);
      wq = q >> 1;
      hasw = (q & 1) == 0;
    } else {
      wq = q;
      hasw = true;
    }
    hasw = hasw && inrow && wq < Wn;

    const bool last = t == p.n_steps - 1;
    const bool rec = (t + 1) % p.record_every == 0;
    const size_t k = rec ? (size_t)((t + 1) / p.record_every - 1) : 0;
    const size_t gr = (k * B + b) * N + row;

    if (hasw) {
      if (rec && p.rec_bits) p.rec_bits[gr * Wn + wq] = word;
      if (last && a.adj_bits) a.adj_bits[g * Wn + wq] = word;
    }
    // tap 0 of the new state (every thread of the row holds the same bits)
    z[0] = static_cast<float>(f0);
    z[1] = static_cast<float>(f1);
    z[2] = static_cast<float>(f2);
    z[3] = static_cast<float>(f3);
    z[4] = static_cast<float>(f4);
    z[5] = static_cast<float>(f5);
    if (owner) {
      const double p2 = a.centralized ? Nd * me.vx - Sv.x : f0;
      const double p3 = a.centralized ? Nd * me.vy - Sv.y : f3;
      u.x = clip10(-gx - p2) / a.action_scalar;
      u.y = clip10(-p3 - gy) / a.action_scalar;
      for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0 ? !rec : !last) continue;
        const size_t d = pass == 0 ? gr : g;
        double* xd = pass == 0 ? p.rec_x : a.x_out;
        float* svd = pass == 0 ? p.rec_sv : a.state_values;
        int32_t* dd = pass == 0 ? p.rec_deg : a.degree_out;
        double* cd = pass == 0 ? p.rec_ctrl : a.ctrl_out;
        if (xd) {
          double2* xo = reinterpret_cast<double2*>(xd) + 2 * d;
          xo[0] = double2{me.px, me.py};
          xo[1] = double2{me.vx, me.vy};
        }
        if (svd) {
          float2* so = reinterpret_cast<float2*>(svd + d * 6);
          so[0] = float2{z[0], z[1]};
          so[1] = float2{z[2], z[3]};
          so[2] = float2{z[4], z[5]};
        }
        if (dd) dd[d] = deg;
        if (cd) reinterpret_cast<double2*>(cd)[d] = u;
      }
    }

    // pass 3: taps 1 .. K-1 of the new state from the previous state's taps 0 .. K-2 of the
    // adjacent columns
    if (K > 1) {
      double s[kZ - 6];
#pragma unroll
      for (int i = 0; i < kZ - 6; ++i) s[i] = 0.0;
      while (ma) {
        const int c = __builtin_ctzll(ma);
        ma &= ma - 1;
        const float2* zr = reinterpret_cast<const float2*>(tprev + (size_t)(jb + c) * TS);
#pragma unroll
        for (int kk = 0; kk < kPolicyMaxTaps - 1; ++kk)
          if (kk < K - 1) {
#pragma unroll
            for (int h = 0; h < 3; ++h) {
              const float2 v = zr[3 * kk + h];
              s[6 * kk + 2 * h] += static_cast<double>(v.x);
              s[6 * kk + 2 * h + 1] += static_cast<double>(v.y);
            }
          }
      }
      const double dn = static_cast<double>(a.mean_pooling ? (deg > 1 ? deg : 1) : 1);
#pragma unroll
      for (int kk = 0; kk < kPolicyMaxTaps - 1; ++kk)
        if (kk < K - 1) {
#pragma unroll
          for (int f = 0; f < 6; ++f) z[6 * (kk + 1) + f] = static_cast<float>(row_sum4(s[6 * kk + f]) / dn);
        }
    }
    if (owner) {
      float2* tw = reinterpret_cast<float2*>(tnext + (size_t)row * TS);
      float2* ar = rec && pa.rec_agg ? reinterpret_cast<float2*>(pa.rec_agg + gr * (size_t)(6 * K)) : nullptr;
      float2* ho = last && pa.taps ? reinterpret_cast<float2*>(pa.taps + g * TS) : nullptr;
#pragma unroll
      for (int kk = 0; kk < kPolicyMaxTaps; ++kk)
        if (kk < K) {
#pragma unroll
          for (int h = 0; h < 3; ++h) {
            const float2 v{z[6 * kk + 2 * h], z[6 * kk + 2 * h + 1]};
            if (kk < K - 1) tw[3 * kk + h] = v;
            if (ar) ar[3 * kk + h] = v;
            if (ho && kk > 0) ho[3 * (kk - 1) + h] = v;
          }
        }
    }
    rec_prev = rec;
    gr_prev = gr;
    ue = ue_next;
  }
  __syncthreads();  // the last step's squared deviations
  if (wid == 0) emit_reward(p.n_steps - 1);
}

template <int CB>
hipError_t launch_cb(const PolicyRolloutArgs& p, size_t lds, hipStream_t s) {
  const dim3 grid(p.r.s.B), block((p.r.s.N * 4 + 63) / 64 * 64);
  if (lds > 64 * 1024) {
    // (per device: set again by every such launch)
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&flock_policy_rollout_kernel<CB>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPolicyLdsMax);
        e != hipSuccess)
      return e;
  }
  hipLaunchKernelGGL((flock_policy_rollout_kernel<CB>), grid, block, lds, s, p);
  return hipGetLastError();
}

// hidden layer l: Pw outputs per thread, padded to PS
inline int padded_quarter(int w_out) { return ((w_out / 4 + 3) / 4) * 4; }

}  // namespace

size_t policy_rollout_lds_bytes(int N, int n_taps, int image_floats) {
  return kLdsFixed + (size_t)((image_floats + 3) & ~3) * sizeof(float) + 2 * (size_t)N * (n_taps - 1) * 6 * sizeof(float);
}

int policy_image_floats(int n_layers, const int* width, int* off_w, int* off_b) {
  int n = 0;
  for (int l = 0; l < n_layers; ++l) {
    const int per_in = l == n_layers - 1 ? 4 : 4 * padded_quarter(width[l + 1]);
    if (off_w) off_w[l] = n;
    n += width[l] * per_in;
    if (off_b) off_b[l] = n;
    n += per_in;
  }
  return n;
}

void policy_pack_image(int n_layers, const int* width, const float* const* weight, const float* const* bias,
                       float* image) {
  int off_w[kPolicyMaxLayers], off_b[kPolicyMaxLayers];
  const int n = policy_image_floats(n_layers, width, off_w, off_b);
  for (int i = 0; i < n; ++i) image[i] = 0.f;
  for (int l = 0; l < n_layers; ++l) {
    const int n_in = width[l], n_out = width[l + 1];
    const bool lastl = l == n_layers - 1;
    const int Pw = lastl ? 1 : n_out / 4, PS = lastl ? 1 : padded_quarter(n_out);
    for (int o = 0; o < n_out; ++o) {
      const int col = (o / Pw) * PS + o % Pw;  // thread o / Pw, its output o % Pw
      for (int i = 0; i < n_in; ++i) image[off_w[l] + i * 4 * PS + col] = weight[l][(size_t)o * n_in + i];
      image[off_b[l] + col] = bias[l][o];
    }
  }
}

hipError_t launch_policy_rollout(const PolicyRolloutArgs& p, hipStream_t s) {
  const int N = p.r.s.N, K = p.net.n_taps;
  if (N < 1 || N > kRolloutMaxN || p.r.s.B < 1 || p.r.n_steps < 1 || p.r.record_every < 1) return hipErrorInvalidValue;
  if (K < 1 || K > kPolicyMaxTaps || p.net.n_layers < 1 || p.net.n_layers > kPolicyMaxLayers) return hipErrorInvalidValue;
  if (K > 1 && !p.taps) return hipErrorInvalidValue;
  const size_t lds = policy_rollout_lds_bytes(N, K, p.net.n_floats);
  if (lds > kPolicyLdsMax) return hipErrorInvalidValue;
  switch (rollout_chunk_bits(N)) {
    case 16: return launch_cb<16>(p, lds, s);
    case 32: return launch_cb<32>(p, lds, s);
    default: return launch_cb<64>(p, lds, s);
  }
}

}  // namespace gf
