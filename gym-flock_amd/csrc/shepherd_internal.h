// Shepherding-v0's device code shared by shep_kernel (shepherd.hip) and the reset and
// recorded-rollout kernels (shepherd_rollout.hip): the launch arguments, the handle, the
// line-of-sight test, and shep_kernel's step as inline functions (the shepherd controller,
// the sheep sum in j order, the unicycle update, the reward, the observation tail), which
// the reset and rollout kernels are built from. shep_kernel itself keeps the same
// statements written out (shepherd.hip says why); with -ffp-contract=off both forms round
// alike, and the GPU tests hold them equal bit for bit. Line numbers are the reference's
// gym_flock/envs/shepherding/shepherding.py.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "capi_common.h"
#include "mt19937.h"

namespace gf {
namespace shep {

constexpr int kWaveEnvs = 4;      // envs per workgroup in the wave-per-env shape
constexpr int kMaxAgents = 1024;  // one workgroup per env above 64 agents

enum ShepMode { M_OBSERVE = 0, M_STEP = 1, M_CONTROLLER = 2, M_ROLLOUT = 3 };

struct ShepArgs {
  int B = 0, N = 0, nsh = 0;
  int mode = 0, n_steps = 0;
  int u_f64 = 0;             // the actions at u are float64 (else float32)
  double dt = 0, comm_r2 = 0, action_scalar = 0;
  double w_shep = 0, w_sheep = 0, goal_r = 0;
  double los2 = 0, los5 = 0;  // np.deg2rad(2), np.deg2rad(5)
  double* x = nullptr;        // (B,N,3)
  double* obs = nullptr;      // (B,N,4)
  double* adj = nullptr;      // (B,N,N)
  double* rew = nullptr;      // (B)
  double* ctrl = nullptr;     // (B,N,2) the control of the last step, all agents
  const void* u = nullptr;    // (B,nsh,2) shepherd actions (M_STEP)
  double* uout = nullptr;     // (B,nsh,2) controller output (M_CONTROLLER)
  double* rew_steps = nullptr;  // (n_steps,B) or null (M_ROLLOUT)
};

// shep_reset_kernel and shep_rollout_kernel (shepherd_rollout.hip)
struct ShepRollArgs {
  int n_steps = 0, every = 1;
  int L = 0;                  // episode length, 0: never reset
  int f32 = 0;                // obs, adj and actions records are float32 (else float64)
  double r_max = 0, off0 = 0, off1 = 0;  // the reset's disk and goal_offset
  uint32_t* mt_key = nullptr;  // (B,624) the envs' streams
  int32_t* mt_pos = nullptr;   // (B)
  const int32_t* count0 = nullptr;  // (B) episode step counts before the launch (L > 0)
  void* obs = nullptr;         // records, each may be null
  void* adj = nullptr;
  void* actions = nullptr;
  double* rewards = nullptr;
  uint8_t* done = nullptr;
  int32_t* n_resets = nullptr;
  // shep_reset_kernel
  const uint8_t* mask = nullptr;  // (B) or null: all
  int seeded = 0, zero_headings = 0;
  uint32_t seed0 = 0;
};

// _wrapToPi :235-238 of atan2(v) - heading, against a threshold (:240-273)
__device__ inline bool in_los(double xs, double ys, double ths, double xt, double yt, double thr) {
  const double vx = xt - xs, vy = yt - ys;
  const double a = atan2(vy, vx) - ths;
  const double dth = a == 0.0 ? 0.0 : atan2(sin(a), cos(a));
  return fabs(dth) < thr;
}

__device__ inline bool all_nonzero(double x, double y, double th) { return x != 0.0 && y != 0.0 && th != 0.0; }

// A thread's place in a launch of either shape, and its env's LDS slots.
template <bool WAVE>
struct Lane {
  static constexpr int S = WAVE ? 64 : kMaxAgents;  // agents per LDS slot
  int e, i, G;  // env slot of the workgroup, agent, the env's lanes
  int64_t b;    // env
  bool active, valid;
  double *sx, *sy, *sth;
  int* flag;
  __device__ __forceinline__ Lane(const ShepArgs& a, double* s_state, int* s_flag) {
    e = WAVE ? (int)(threadIdx.x >> 6) : 0;
    i = WAVE ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    G = WAVE ? 64 : (int)blockDim.x;
    b = WAVE ? (int64_t)blockIdx.x * kWaveEnvs + e : (int64_t)blockIdx.x;
    active = b < a.B;
    valid = active && i < a.N;
    sx = s_state + e * 3 * S;
    sy = sx + S;
    sth = sy + S;
    flag = s_flag + e * S;
  }
};

// controller() :204-233 of the state in LDS: (vx, vy) of shepherd lane i (other lanes keep
// theirs). The line-of-sight tests of all (shepherd, agent) pairs are spread over the env's
// lanes; bit 0: a sheep in sight, bit 1: a shepherd in sight. Two workgroup barriers: every
// thread of the workgroup calls it.
template <bool WAVE>
__device__ __forceinline__ void controller_out(const ShepArgs& a, const Lane<WAVE>& l, double xi, double yi, double ti,
                                               double c, double s, double& vx, double& vy) {
  const int N = a.N, nsh = a.nsh, i = l.i;
  const double *sx = l.sx, *sy = l.sy, *sth = l.sth;
  int* flag = l.flag;
  if (l.valid && i < nsh) flag[i] = 0;
  __syncthreads();
  if (l.active) {
    for (int p = i; p < nsh * N; p += l.G) {
      const int k = p / N, j = p - k * N;
      const double xs = sx[k], ys = sy[k], ths = sth[k];
      if (j >= nsh) {
        if (in_los(xs, ys, ths, sx[j], sy[j], a.los2)) atomicOr(&flag[k], 1);
      } else if (all_nonzero(xs, ys, ths) != all_nonzero(sx[j], sy[j], sth[j])) {
        // :253 compares s.all() with shepherd.all(): a shepherd is tested only when
        // exactly one of the two states has a zero component
        if (in_los(xs, ys, ths, sx[j], sy[j], a.los2)) atomicOr(&flag[k], 2);
      }
    }
  }
  __syncthreads();
  if (l.valid && i < nsh) {
    const int f = flag[i];
    double vl, vr;
    if (f & 1) {
      vl = 0.0082, vr = 0.9996;
    } else if (f & 2) {
      vl = 0.5471, vr = 0.6098;
    } else if (in_los(xi, yi, ti, 0.0, 0.0, a.los5)) {
      vl = 0.9993, vr = 0.9447;
    } else {
      vl = 0.9998, vr = 0.8520;
    }
    const double v = (vr + vl) / 2;
    const double wd = ((vr - vl) / 0.6) * 0.3;
    vx = v * c - wd * s;
    vy = v * s + wd * c;
  }
}

// _compute_sheep_controller :164-178 of sheep i, j in order
__device__ __forceinline__ void sheep_sum(const ShepArgs& a, int i, const double* sx, const double* sy, double xi,
                                          double yi, double& ux, double& uy) {
  const int N = a.N, nsh = a.nsh;
  for (int j = 0; j < N; ++j) {
    const double dx = xi - sx[j], dy = yi - sy[j];
    double r2 = dx * dx + dy * dy;
    if (r2 > 2.0 || j == i) r2 = __builtin_inf();
    const double w = j < nsh ? a.w_shep : a.w_sheep;
    const double tx = w * (dx / r2), ty = w * (dy / r2);
    ux = j == 0 ? tx : ux + tx;
    uy = j == 0 ? ty : uy + ty;
  }
}

// feedback linearisation and the unicycle update :106-115
__device__ __forceinline__ void unicycle(const ShepArgs& a, bool sheep, double c, double s, double ux, double uy,
                                         double& xi, double& yi, double& ti) {
  double v = ux * c + uy * s;
  const double w = ux * (-s / 0.3) + uy * (c / 0.3);
  if (sheep) v = v / 2 + 0.5;
  xi = xi + v * c * a.dt;
  yi = yi + v * s * a.dt;
  ti = ti + w * a.dt;
}

// reward :180-185: the sheep inside the goal circle, counted over the env's lanes (a
// workgroup barrier in the workgroup shape: every thread calls it)
template <bool WAVE>
__device__ __forceinline__ double reward_of(const ShepArgs& a, const Lane<WAVE>& l, double xi, double yi) {
  const bool in_goal = l.valid && l.i >= a.nsh && sqrt(xi * xi + yi * yi) < a.goal_r;
  const int cnt = WAVE ? __popcll(__ballot(in_goal)) : __syncthreads_count(in_goal);
  return (double)cnt / (double)(a.N - a.nsh);
}

// observation row :127 of agent i
template <class T>
__device__ __forceinline__ void write_obs(T* o, int i, int nsh, double xi, double yi, double ti) {
  o[0] = (T)xi;
  o[1] = (T)yi;
  o[2] = (T)ti;
  o[3] = i < nsh ? (T)1.0 : (T)0.0;
}

// adjacency :139-162 of the state in LDS: lane i holds column i, so a row's N values go out
// as one contiguous store. adj: the env's (N,N) block.
template <class T>
__device__ __forceinline__ void write_adj(T* adj, const ShepArgs& a, int i, const double* sx, const double* sy,
                                          double xi, double yi) {
  const int N = a.N;
  T* row = adj + i;
  for (int r = 0; r < N; ++r) {
    const double dx = sx[r] - xi, dy = sy[r] - yi;
    const double r2 = dx * dx + dy * dy;
    row[(size_t)r * N] = (T)((r != i && r2 < a.comm_r2) ? 1.0 / sqrt(r2) : 0.0);
  }
}

}  // namespace shep
}  // namespace gf

struct shep_handle {
  shep_config cfg{};
  hipStream_t stream = nullptr;
  gf::shep::ShepArgs a{};
  double* ubuf = nullptr;     // (B,nsh,2) doubles: the resident actions (float32 ones use half)
  double* rew_steps = nullptr;
  size_t rew_steps_cap = 0;   // in doubles
  void* scratch = nullptr;    // float32 casts on their way to host memory
  size_t scratch_cap = 0;
  bool has_state = false, has_obs = false, has_ctrl = false, has_u = false;
  int u_f64 = 0;              // dtype of the resident actions
  // shepherd_rollout.hip: the envs' MT19937 streams (allocated on first use), the episode
  // step counts (kept on the host; a rollout with resets uploads them), and the records of
  // a rollout on their way to host memory
  uint32_t* mt_key = nullptr;  // (B,624)
  int32_t* mt_pos = nullptr;   // (B)
  std::vector<uint8_t> rng_set;    // (B) the env's stream was seeded or set
  std::vector<int32_t> ep_count;   // (B)
  int32_t* count_dev = nullptr;    // (B)
  uint8_t* mask_dev = nullptr;     // (B) shep_reset_device's selection
  unsigned char* rec = nullptr;
  size_t rec_cap = 0;              // in bytes

  // every stepping call advances the episode step counts
  void count_steps(int n) {
    for (int32_t& c : ep_count) c = (int32_t)std::min<int64_t>((int64_t)c + n, (int64_t)1 << 30);
  }
};
