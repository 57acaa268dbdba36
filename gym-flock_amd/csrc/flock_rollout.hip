// Closed-loop expert rollout of FlockingRelative (and its variants) in one launch:
// n_steps of `u = env.controller(); env.step(u)` (flocking_relative.py:91-109, :194-226)
// for every env, optionally recording every record_every-th step.
//
// One workgroup owns one env of N <= kRolloutMaxN agents for the whole rollout, four
// threads per agent (4N threads, rounded up to whole waves). The env's float64 state lives
// in LDS (32 B per agent, two copies: step t + 1 is published while stragglers still read
// step t); each agent's state and its latest control also stay in the registers of the
// agent's owner thread, which applies the dynamics (flock_dynamics.h, the step kernels'
// own arithmetic) without a memory round trip. Nothing is read from global memory after
// the first step (with a per-step dt table, RolloutArgs.dt_steps: one 8-byte value per
// step, loaded a step ahead), and nothing is written but the records and, by the last
// step, the handle's buffers.
//
// Thread q of row i owns the columns [q * CB, (q + 1) * CB), CB = 16, 32 or 64 for
// N <= 64, 128, 256: a quarter of the row's adjacency bits in fe_get_network_packed's
// order. A step has two passes over them, both in float64 with r2 = dx*dx + dy*dy
// uncontracted (this file is built with -ffp-contract=off like flock_kernels.hip):
//   pass 1  every column: one compare, !(r2 > max(comm_radius, comm_radius^2)), marks the
//           candidates in a register: every neighbour (r2 < comm_radius^2, :117), every
//           pair inside the controller's mask (not r2 > comm_radius, :225) and every pair
//           whose r2 is NaN.
//   pass 2  the candidates only (a few per row): both decisions exactly, the one IEEE
//           division, features, gradient and adjacency bits.
//
// Summation order (deterministic, no atomics): a thread adds its candidates in ascending
// j; the four threads of a row are combined by an xor butterfly (distance 1, then 2),
// every lane of the row ending with the same bits. The sums over the env's agents (the
// velocity sums of the centralised controller and the reward, and the reward's squared
// deviations) are a wave butterfly followed by a fixed pairwise tree over the 16 wave
// slots. The order depends on N only, never on the batch, the launch, n_steps or
// record_every. The centralised velocity term is N v_i - sum_j v_j, as in the step kernel
// (step_epilogue).
//
// A step has ONE workgroup barrier, after the owners publish the new state and the waves'
// velocity sums. Everything a later step overwrites is double-buffered by the step's
// parity (state, both sets of wave slots), and step t's reward is summed by wave 0 after
// step t + 1's barrier. No other synchronisation: workgroups never look at each other.
#include "flock_dynamics.h"
#include "flock_internal.h"
#include "flock_rollout_shared.h"

namespace gf {

namespace {

template <int CB, bool VAR>
__global__ __launch_bounds__(kRolloutThreads) void flock_rollout_kernel(RolloutArgs p) {
  const StepArgs& a = p.s;
  // by the step's parity: the state; per wave the (vx, vy) sums and the squared deviations
  __shared__ St st[2][kRolloutMaxN];
  __shared__ double2 red1[2][kRolloutWaves], red2[2][kRolloutWaves];

  const int N = a.N, B = a.B, b = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int Wn = (N + 63) >> 6;
  // 4 threads per row, thread q over columns [q * CB, (q + 1) * CB)
  const int row = tid >> 2, q = tid & 3;
  const bool inrow = row < N;
  const bool owner = q == 0 && inrow;
  const int jb = q * CB;
  const size_t g = (size_t)b * N + row;  // this row's index in the handle's (B,N,.) buffers
  const double Nd = static_cast<double>(N);
  const double tmax = a.cr > a.cr2 ? a.cr : a.cr2;
  double dt = a.dt;
  if constexpr (VAR) {
    // the per-step table's first row, or the launch's per-env dt
    const double* dt0 = p.dt_steps ? p.dt_steps : a.dt_env;
    if (dt0) dt = dt0[b];
  }
  if (tid < 2 * kRolloutWaves) {  // the slots of waves past the block's stay 0
    red1[tid >> 4][tid & 15] = double2{0.0, 0.0};
    red2[tid >> 4][tid & 15] = double2{0.0, 0.0};
  }
  __syncthreads();

  St me{0.0, 0.0, 0.0, 0.0};
  double2 u{0.0, 0.0};
  if (owner) {
    const double2* xp = reinterpret_cast<const double2*>(a.x_in) + 2 * g;
    const double2 pp = xp[0], vv = xp[1];
    me = St{pp.x, pp.y, vv.x, vv.y};
    u = reinterpret_cast<const double2*>(a.u)[g];
  }

  // step t's reward from its squared deviations (wave 0, after a barrier that follows them)
  auto emit_reward = [&](int t) {
    const double2 Q = slot_sum(red2[t & 1], lane);
    if (tid == 0) {
      const double rw = -1.0 * (Q.x / Nd + Q.y / Nd);
      if (p.rec_rewards) p.rec_rewards[(size_t)t * B + b] = rw;
      if (t == p.n_steps - 1 && a.reward) a.reward[b] = rw;
    }
  };

  for (int t = 0; t < p.n_steps; ++t) {
    St* cur = st[t & 1];
    // the next step's dt (fe_set_dt_noise), loaded a step ahead: the one global read of a step
    double dt_next = dt;
    if constexpr (VAR) {
      if (p.dt_steps && t + 1 < p.n_steps) dt_next = p.dt_steps[(size_t)(t + 1) * B + b];
      // held in vector registers across the step: the scalar file is full (the value is
      // the same in every lane)
      asm volatile("" : "+v"(dt_next));
    }
    // dynamics: the owner's registers hold the agent's state and its control
    if (owner) {
      const double2 pp{me.px, me.py}, vv{me.vx, me.vy};
      if constexpr (VAR) me = integrate_variant<true>(a, dt, row, pp, vv, u);
      else me = integrate_plain<true>(a, pp, vv, u);
      cur[row] = me;
    }
    {
      const double sx = wave_sum64(owner ? me.vx : 0.0), sy = wave_sum64(owner ? me.vy : 0.0);
      if (lane == 0) red1[t & 1][wid] = double2{sx, sy};
    }
    __syncthreads();  // the step's state and velocity sums are in LDS
    if (wid == 0 && t > 0) emit_reward(t - 1);

    // the env's velocity sums: the centralised controller's and the reward's mean
    // (instant_cost :145-147 = -(var(vx) + var(vy)), two-pass like np.var)
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
        // (columns past N - 1 read LDS the env does not use: masked below)
        const double2 pj = *reinterpret_cast<const double2*>(&cur[(jb + c) & (kRolloutMaxN - 1)]);
        const double dx = r.px - pj.x, dy = r.py - pj.y;
        const double r2 = dx * dx + dy * dy;
        mc |= !(r2 > tmax) ? (1ull << c) : 0ull;
      }
      const int nv = N - jb;  // valid columns of this thread
      mc &= nv >= 64 ? ~0ull : (nv > 0 ? (1ull << nv) - 1ull : 0ull);
      const int dg = row - jb;  // the diagonal (:115): no neighbour, no gradient
      if (dg >= 0 && dg < CB) mc &= ~(1ull << dg);
    }

    // pass 2: compute_helpers (:111-134) and controller (:194-226) over the candidates
    double f0 = 0, f1 = 0, f2 = 0, f3 = 0, f4 = 0, f5 = 0, gx = 0, gy = 0;
    uint64_t ma = 0;  // adjacency bits of this thread's CB columns
    {
      while (mc) {
        const int c = __builtin_ctzll(mc);
        mc &= mc - 1;
        const int j = jb + c;
        const St o = cur[j];
        const double dx = r.px - o.px, dy = r.py - o.py;
        const double r2 = dx * dx + dy * dy;
        const bool isadj = r2 < a.cr2;  // :117, strict
        const bool far = r2 > a.cr;     // :225 (comm_radius, not its square); a NaN r2 is not far
        const double ir = 1.0 / r2, irr = ir * ir;
        const double q1x = dx * irr, q2x = dx * ir;
        const double q1y = dy * irr, q2y = dy * ir;
        if (isadj) {
          // obstacle variant: no velocity difference for pairs touching agents < n_vel_zero
          const bool vz = VAR && (row < a.n_vel_zero || j < a.n_vel_zero);
          ma |= 1ull << c;
          f0 += vz ? 0.0 : r.vx - o.vx;
          f1 += q1x;
          f2 += q2x;
          f3 += vz ? 0.0 : r.vy - o.vy;
          f4 += q1y;
          f5 += q2y;
        }
        if (!far && (a.centralized || isadj)) {
          gx += (-2.0 * q1x) + (2.0 * q2x);
          gy += (-2.0 * q1y) + (2.0 * q2y);
        }
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
    // the row's adjacency words: `word` is word `wq` of the row in the lanes with `hasw`
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
    const size_t gr = (k * B + b) * N + row;  // this row in the (K,B,N,.) records

    if (hasw) {
      if (rec && p.rec_bits) p.rec_bits[gr * Wn + wq] = word;
      if (last && a.adj_bits) a.adj_bits[g * Wn + wq] = word;
    }
    if (owner) {
      // centralized: sum over ALL j of (v_i - v_j) = N*v_i - sum_j v_j (:200-208)
      double p2 = a.centralized ? Nd * me.vx - Sv.x : f0;
      double p3 = a.centralized ? Nd * me.vy - Sv.y : f3;
      if (VAR && a.centralized && a.n_vel_zero > 0) {
        // obstacle variant: only pairs between free agents count (flocking_obstacle.py:79-80)
        const int nz = min(a.n_vel_zero, N);
        double zx = 0, zy = 0;
        for (int j = 0; j < nz; ++j) {
          zx += cur[j].vx;
          zy += cur[j].vy;
        }
        const bool frozen = row < nz;
        p2 = frozen ? 0.0 : static_cast<double>(N - nz) * me.vx - (Sv.x - zx);
        p3 = frozen ? 0.0 : static_cast<double>(N - nz) * me.vy - (Sv.y - zy);
      }
      u.x = clip10(-gx - p2) / a.action_scalar;  // (-p4 - p2), :209-211
      u.y = clip10(-p3 - gy) / a.action_scalar;  // (-p3 - p5)
      if (VAR && a.ctrl_clip > 0) {  // stochastic variant (flocking_stoch.py:44-45)
        u.x = clip_sym(u.x, a.ctrl_clip);
        u.y = clip_sym(u.y, a.ctrl_clip);
      }
      const float2 sv0{static_cast<float>(f0), static_cast<float>(f1)};
      const float2 sv1{static_cast<float>(f2), static_cast<float>(f3)};
      const float2 sv2{static_cast<float>(f4), static_cast<float>(f5)};
      // one destination set per pass: the record (rec) and the handle's buffers (last)
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
        if (svd) {  // 24-byte rows: 8-byte stores
          float2* so = reinterpret_cast<float2*>(svd + d * 6);
          so[0] = sv0;
          so[1] = sv1;
          so[2] = sv2;
        }
        if (dd) dd[d] = deg;
        if (cd) reinterpret_cast<double2*>(cd)[d] = u;
      }
    }
    if constexpr (VAR) dt = dt_next;
  }
  __syncthreads();  // the last step's squared deviations
  if (wid == 0) emit_reward(p.n_steps - 1);
}

template <int CB>
hipError_t launch_cb(const RolloutArgs& p, hipStream_t s) {
  const dim3 grid(p.s.B), block((p.s.N * 4 + 63) / 64 * 64);
  if (p.s.variant) hipLaunchKernelGGL((flock_rollout_kernel<CB, true>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((flock_rollout_kernel<CB, false>), grid, block, 0, s, p);
  return hipGetLastError();
}

}  // namespace

int rollout_chunk_bits(int N) { return N <= 64 ? 16 : (N <= 128 ? 32 : 64); }

hipError_t launch_rollout(const RolloutArgs& p, hipStream_t s) {
  if (p.s.N < 1 || p.s.N > kRolloutMaxN || p.s.B < 1 || p.n_steps < 1 || p.record_every < 1) return hipErrorInvalidValue;
  switch (rollout_chunk_bits(p.s.N)) {
    case 16: return launch_cb<16>(p, s);
    case 32: return launch_cb<32>(p, s);
    default: return launch_cb<64>(p, s);
  }
}

}  // namespace gf
