// Shepherding-v0 on the device (reference gym_flock/envs/shepherding/shepherding.py):
// step :80-117 with the sheep controller :164-178, observation :127, weighted adjacency
// :139-162, reward :180-185 and the heuristic shepherd controller :204-273; C-ABI shep_*
// (include/gymflock.h).
//
// One lane owns one agent. An env's state (N,3) float64 lives in LDS for the whole
// launch, so a closed-loop rollout of n steps touches global memory for the state once
// in and once out. Two launch shapes:
//   N <= 64        one wave per env, four envs per 256-thread workgroup (the last
//                  workgroup of a batch may hold empty waves; they only keep the barriers)
//   64 < N <= 1024 one workgroup per env, ceil(N / 64) waves
//
// The sheep repulsion of agent i is the reference's np.sum(force_weights * (diff / r2),
// axis=1): NumPy reduces the middle axis of the (N,N,2) array one j after the other, so
// the sum here runs j = 0 .. N-1 in order on lane i (each x_j, y_j one LDS broadcast
// read), starting from the j = 0 term. A tree or cross-lane reduction rounds differently.
// -ffp-contract=off (csrc/Makefile) keeps dx*dx + dy*dy and every a*b + c unfused, as
// NumPy computes them.
//
// cos / sin / atan2 are the device library's; they are not NumPy's to the last bit, so
// free-running trajectories match the reference to rounding. The adjacency, the reward
// and the sheep controls contain no trigonometry and are bit-exact for the same state.
//
// The launch arguments, the handle and the line-of-sight test are shepherd_internal.h's,
// shared with the reset and recorded-rollout kernels of shepherd_rollout.hip. That header
// also holds this kernel's step as inline functions (controller_out, sheep_sum, unicycle,
// reward_of, write_obs, write_adj), which those kernels call. shep_kernel keeps the step
// written out below, statement for statement the same arithmetic: built from the
// functions it had the same registers and five instructions fewer, yet measured 2 % slower
// per step at 512 envs (9.74 against 9.53 us in 100-step launches, three alternating runs
// each), so its text stays. tests/test_shepherding_rollout_gpu.py holds the two forms
// equal bit for bit (a rollout against step(expert=True) and against expert_steps).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "capi_common.h"
#include "shepherd_internal.h"

using gf::dalloc;
using gf::fail;
using namespace gf::shep;

namespace {

template <bool WAVE>
__global__ __launch_bounds__(WAVE ? 64 * kWaveEnvs : kMaxAgents) void shep_kernel(ShepArgs a) {
  constexpr int S = WAVE ? 64 : kMaxAgents;  // agents per LDS slot
  __shared__ double s_state[(WAVE ? kWaveEnvs : 1) * 3 * S];
  __shared__ int s_flag[(WAVE ? kWaveEnvs : 1) * S];
  const int e = WAVE ? (int)(threadIdx.x >> 6) : 0;
  const int i = WAVE ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  const int G = WAVE ? 64 : (int)blockDim.x;
  const int64_t b = WAVE ? (int64_t)blockIdx.x * kWaveEnvs + e : (int64_t)blockIdx.x;
  const int N = a.N, nsh = a.nsh;
  const bool active = b < a.B;
  const bool valid = active && i < N;
  double* sx = s_state + e * 3 * S;
  double* sy = sx + S;
  double* sth = sy + S;
  int* flag = s_flag + e * S;

  double xi = 0, yi = 0, ti = 0;
  if (valid) {
    const double* p = a.x + ((size_t)b * N + i) * 3;
    xi = p[0];
    yi = p[1];
    ti = p[2];
    sx[i] = xi;
    sy[i] = yi;
    sth[i] = ti;
  }
  __syncthreads();

  const bool with_ctrl = a.mode == M_CONTROLLER || a.mode == M_ROLLOUT;
  const int steps = a.mode == M_ROLLOUT ? a.n_steps : (a.mode == M_OBSERVE ? 0 : 1);
  for (int t = 0; t < steps; ++t) {
    double c = 0, s = 0, ux = 0, uy = 0;
    if (valid) {
      c = cos(ti);
      s = sin(ti);
    }
    if (with_ctrl) {
      // controller() :204-233. The line-of-sight tests of all (shepherd, agent) pairs are
      // spread over the env's lanes; bit 0: a sheep in sight, bit 1: a shepherd in sight
      if (valid && i < nsh) flag[i] = 0;
      __syncthreads();
      if (active) {
        for (int p = i; p < nsh * N; p += G) {
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
      if (valid && i < nsh) {
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
        const double vx = v * c - wd * s;
        const double vy = v * s + wd * c;
        if (a.mode == M_CONTROLLER) {
          double* o = a.uout + ((size_t)b * nsh + i) * 2;
          o[0] = vx;
          o[1] = vy;
        }
        ux = vx * a.action_scalar;
        uy = vy * a.action_scalar;
      }
      if (a.mode == M_CONTROLLER) break;
    } else if (valid && i < nsh) {
      // u * action_scalar :89 in the actions' own precision
      const size_t o = ((size_t)b * nsh + i) * 2;
      if (a.u_f64) {
        const double* u = static_cast<const double*>(a.u);
        ux = u[o] * a.action_scalar;
        uy = u[o + 1] * a.action_scalar;
      } else {
        const float* u = static_cast<const float*>(a.u);
        const float sc = (float)a.action_scalar;
        ux = (double)(u[o] * sc);
        uy = (double)(u[o + 1] * sc);
      }
    }
    if (valid && i >= nsh) {
      // _compute_sheep_controller :164-178, j in order
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
    if (valid) {
      // feedback linearisation and the unicycle update :106-115
      double v = ux * c + uy * s;
      const double w = ux * (-s / 0.3) + uy * (c / 0.3);
      if (i >= nsh) v = v / 2 + 0.5;
      xi = xi + v * c * a.dt;
      yi = yi + v * s * a.dt;
      ti = ti + w * a.dt;
      if (t == steps - 1) {
        double* o = a.ctrl + ((size_t)b * N + i) * 2;
        o[0] = ux;
        o[1] = uy;
      }
    }
    __syncthreads();  // every read of the old state is done
    if (valid) {
      sx[i] = xi;
      sy[i] = yi;
      sth[i] = ti;
    }
    __syncthreads();
    if (a.rew_steps) {
      const bool in_goal = valid && i >= nsh && sqrt(xi * xi + yi * yi) < a.goal_r;
      const int cnt = WAVE ? __popcll(__ballot(in_goal)) : __syncthreads_count(in_goal);
      if (active && i == 0) a.rew_steps[(size_t)t * a.B + b] = (double)cnt / (double)(N - nsh);
    }
  }
  if (a.mode == M_CONTROLLER) return;

  // observation :127, adjacency :139-162 and reward :180-185 of the state now in LDS
  {
    const bool in_goal = valid && i >= nsh && sqrt(xi * xi + yi * yi) < a.goal_r;
    const int cnt = WAVE ? __popcll(__ballot(in_goal)) : __syncthreads_count(in_goal);
    if (active && i == 0) a.rew[b] = (double)cnt / (double)(N - nsh);
  }
  if (valid) {
    double* o = a.obs + ((size_t)b * N + i) * 4;
    o[0] = xi;
    o[1] = yi;
    o[2] = ti;
    o[3] = i < nsh ? 1.0 : 0.0;
    if (a.mode != M_OBSERVE) {
      double* p = a.x + ((size_t)b * N + i) * 3;
      p[0] = xi;
      p[1] = yi;
      p[2] = ti;
    }
    // lane i holds column i: a row's N values go out as one contiguous store
    double* row = a.adj + (size_t)b * N * N + i;
    for (int r = 0; r < N; ++r) {
      const double dx = sx[r] - xi, dy = sy[r] - yi;
      const double r2 = dx * dx + dy * dy;
      row[(size_t)r * N] = (r != i && r2 < a.comm_r2) ? 1.0 / sqrt(r2) : 0.0;
    }
  }
}

__global__ __launch_bounds__(256) void shep_cast_kernel(const double* src, float* dst, size_t n) {
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) dst[k] = (float)src[k];
}

int launch(shep_handle* h, int mode, int n_steps, double* rew_steps) {
  ShepArgs a = h->a;
  a.mode = mode;
  a.n_steps = n_steps;
  a.rew_steps = rew_steps;
  if (a.N <= 64) {
    const unsigned grid = (unsigned)((a.B + kWaveEnvs - 1) / kWaveEnvs);
    shep_kernel<true><<<grid, 64 * kWaveEnvs, 0, h->stream>>>(a);
  } else {
    shep_kernel<false><<<(unsigned)a.B, (unsigned)((a.N + 63) / 64 * 64), 0, h->stream>>>(a);
  }
  GF_HIP(hipGetLastError());
  return GF_OK;
}

// one output buffer of n doubles to dst: host or device memory, float64 or float32
int copy_out(shep_handle* h, const double* src, size_t n, void* dst, int flags) {
  const bool dev = flags & SHEP_OUT_DEVICE, f32 = flags & SHEP_OUT_F32;
  if (!f32) {
    GF_HIP(hipMemcpyAsync(dst, src, n * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                          h->stream));
  } else {
    float* out = static_cast<float*>(dst);
    if (!dev) {
      if (h->scratch_cap < n * sizeof(float)) {
        GF_HIP(hipStreamSynchronize(h->stream));
        if (h->scratch) GF_HIP(hipFree(h->scratch));
        h->scratch = nullptr;
        h->scratch_cap = 0;
        if (int rc = dalloc(reinterpret_cast<unsigned char**>(&h->scratch), n * sizeof(float))) return rc;
        h->scratch_cap = n * sizeof(float);
      }
      out = static_cast<float*>(h->scratch);
    }
    const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    shep_cast_kernel<<<grid, 256, 0, h->stream>>>(src, out, n);
    GF_HIP(hipGetLastError());
    if (!dev) GF_HIP(hipMemcpyAsync(dst, out, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  }
  if (!dev) GF_HIP(hipStreamSynchronize(h->stream));  // device destinations: stream-ordered, shep_sync
  return GF_OK;
}

}  // namespace

extern "C" {

int shep_create(const shep_config* cfg, shep_handle** out) {
  if (!cfg || !out) return fail(GF_EINVAL, "null argument");
  *out = nullptr;
  if (cfg->n_shepherds < 1) return fail(GF_EINVAL, "n_shepherds must be >= 1");
  if (cfg->n_sheep < 1) return fail(GF_EINVAL, "n_sheep must be >= 1");
  if ((int64_t)cfg->n_shepherds + cfg->n_sheep > kMaxAgents)
    return fail(GF_EINVAL, "n_shepherds + n_sheep must be <= 1024");
  if (cfg->n_envs < 1) return fail(GF_EINVAL, "n_envs must be >= 1");
  if (!(cfg->dt > 0)) return fail(GF_EINVAL, "dt must be > 0");
  if (!(cfg->comm_radius > 0)) return fail(GF_EINVAL, "comm_radius must be > 0");
  if (!(cfg->goal_region_radius > 0)) return fail(GF_EINVAL, "goal_region_radius must be > 0");
  if (int rc = gf::select_device(cfg->device)) return rc;
  shep_handle* h = new shep_handle();
  h->cfg = *cfg;
  ShepArgs& a = h->a;
  a.B = cfg->n_envs;
  a.nsh = cfg->n_shepherds;
  a.N = cfg->n_shepherds + cfg->n_sheep;
  a.dt = cfg->dt;
  a.comm_r2 = cfg->comm_radius * cfg->comm_radius;  // comm_radius_2 :47
  a.action_scalar = cfg->action_scalar;
  a.w_shep = cfg->force_weight_shepherd;
  a.w_sheep = cfg->force_weight_sheep;
  a.goal_r = cfg->goal_region_radius;
  a.los2 = 2.0 * (M_PI / 180.0);  // np.deg2rad
  a.los5 = 5.0 * (M_PI / 180.0);
  const size_t BN = (size_t)a.B * a.N;
  int rc = GF_OK;
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) rc = fail(GF_EHIP, "hipStreamCreate");
  if (!rc) rc = dalloc(&a.x, BN * 3);
  // observation, adjacency and rewards in one block: shep_get_outputs is one copy
  if (!rc) rc = dalloc(&a.obs, BN * 4 + BN * a.N + (size_t)a.B);
  if (!rc) {
    a.adj = a.obs + BN * 4;
    a.rew = a.adj + BN * a.N;
  }
  if (!rc) rc = dalloc(&a.ctrl, BN * 2);
  if (!rc) rc = dalloc(&h->ubuf, (size_t)a.B * a.nsh * 2);
  if (rc) {
    shep_destroy(h);
    return rc;
  }
  a.uout = h->ubuf;
  h->ep_count.assign((size_t)a.B, 0);
  h->rng_set.assign((size_t)a.B, 0);
  *out = h;
  return GF_OK;
}

int shep_destroy(shep_handle* h) {
  if (!h) return GF_OK;
  hipSetDevice(h->cfg.device);
  if (h->stream) hipStreamSynchronize(h->stream);
  void* bufs[] = {h->a.x,  h->a.obs,  h->a.ctrl,    h->ubuf,     h->rew_steps, h->scratch,
                  h->mt_key, h->mt_pos, h->count_dev, h->mask_dev, h->rec};
  for (void* p : bufs)
    if (p) hipFree(p);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
  return GF_OK;
}

int shep_set_state(shep_handle* h, const double* x) {
  if (!h || !x) return fail(GF_EINVAL, "null argument");
  GF_HIP(hipSetDevice(h->cfg.device));
  GF_HIP(hipMemcpyAsync(h->a.x, x, sizeof(double) * 3 * h->a.B * h->a.N, hipMemcpyHostToDevice, h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  h->has_state = true;
  h->has_obs = h->has_ctrl = false;
  h->ep_count.assign(h->ep_count.size(), 0);
  return GF_OK;
}

int shep_get_state(shep_handle* h, double* x) {
  if (!h || !x) return fail(GF_EINVAL, "null argument");
  if (!h->has_state) return fail(GF_ESTATE, "set a state first (shep_set_state)");
  GF_HIP(hipSetDevice(h->cfg.device));
  GF_HIP(hipMemcpyAsync(x, h->a.x, sizeof(double) * 3 * h->a.B * h->a.N, hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  return GF_OK;
}

int shep_observe(shep_handle* h) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->has_state) return fail(GF_ESTATE, "set a state first (shep_set_state)");
  GF_HIP(hipSetDevice(h->cfg.device));
  if (int rc = launch(h, M_OBSERVE, 0, nullptr)) return rc;
  h->has_obs = true;
  return GF_OK;
}

int shep_step(shep_handle* h, const void* u, int flags) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (flags & ~(SHEP_U_DEVICE | SHEP_U_F64 | SHEP_U_EXPERT | SHEP_U_RESIDENT)) return fail(GF_EINVAL, "unknown flag");
  if (!h->has_state) return fail(GF_ESTATE, "set a state first (shep_set_state)");
  GF_HIP(hipSetDevice(h->cfg.device));
  ShepArgs& a = h->a;
  int mode = M_STEP;
  if (flags & SHEP_U_EXPERT) {
    mode = M_ROLLOUT;
  } else if (flags & SHEP_U_RESIDENT) {
    if (!h->has_u) return fail(GF_ESTATE, "no resident actions (a host-action shep_step or shep_controller first)");
    a.u = h->ubuf;
    a.u_f64 = h->u_f64;
  } else {
    if (!u) return fail(GF_EINVAL, "null actions");
    const int f64 = (flags & SHEP_U_F64) ? 1 : 0;
    if (flags & SHEP_U_DEVICE) {
      a.u = u;
    } else {
      // pageable host memory: the copy has left the caller's buffer when this returns
      GF_HIP(hipMemcpyAsync(h->ubuf, u, (size_t)a.B * a.nsh * 2 * (f64 ? 8 : 4), hipMemcpyHostToDevice, h->stream));
      a.u = h->ubuf;
      h->has_u = true;
      h->u_f64 = f64;
    }
    a.u_f64 = f64;
  }
  if (int rc = launch(h, mode, 1, nullptr)) return rc;
  h->has_obs = h->has_ctrl = true;
  h->count_steps(1);
  return GF_OK;
}

int shep_controller(shep_handle* h, double* out) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->has_state) return fail(GF_ESTATE, "set a state first (shep_set_state)");
  GF_HIP(hipSetDevice(h->cfg.device));
  if (int rc = launch(h, M_CONTROLLER, 1, nullptr)) return rc;
  h->has_u = true;  // the output is the resident action buffer, float64
  h->u_f64 = 1;
  if (out) {
    GF_HIP(hipMemcpyAsync(out, h->ubuf, sizeof(double) * 2 * h->a.B * h->a.nsh, hipMemcpyDeviceToHost, h->stream));
    GF_HIP(hipStreamSynchronize(h->stream));
  }
  return GF_OK;
}

int shep_step_expert(shep_handle* h, int n_steps, double* rewards) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (n_steps < 1) return fail(GF_EINVAL, "n_steps must be >= 1");
  if (!h->has_state) return fail(GF_ESTATE, "set a state first (shep_set_state)");
  GF_HIP(hipSetDevice(h->cfg.device));
  const size_t n = (size_t)n_steps * h->a.B;
  if (h->rew_steps_cap < n) {
    GF_HIP(hipStreamSynchronize(h->stream));
    if (h->rew_steps) GF_HIP(hipFree(h->rew_steps));
    h->rew_steps = nullptr;
    h->rew_steps_cap = 0;
    if (int rc = dalloc(&h->rew_steps, n)) return rc;
    h->rew_steps_cap = n;
  }
  if (int rc = launch(h, M_ROLLOUT, n_steps, h->rew_steps)) return rc;
  h->has_obs = h->has_ctrl = true;
  h->count_steps(n_steps);
  if (rewards) {
    GF_HIP(hipMemcpyAsync(rewards, h->rew_steps, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    GF_HIP(hipStreamSynchronize(h->stream));
  }
  return GF_OK;
}

// per_env doubles of every env from one of the observation buffers
static int get_out(shep_handle* h, double* const ShepArgs::*buf, size_t per_env, void* dst, int flags) {
  if (!h || !dst) return fail(GF_EINVAL, "null argument");
  if (flags & ~(SHEP_OUT_DEVICE | SHEP_OUT_F32)) return fail(GF_EINVAL, "unknown flag");
  if (!h->has_obs) return fail(GF_ESTATE, "no observation yet (shep_observe or shep_step first)");
  GF_HIP(hipSetDevice(h->cfg.device));
  return copy_out(h, h->a.*buf, (size_t)h->a.B * per_env, dst, flags);
}

int shep_get_obs(shep_handle* h, void* dst, int flags) {
  return get_out(h, &ShepArgs::obs, h ? (size_t)h->a.N * 4 : 0, dst, flags);
}

int shep_get_adj(shep_handle* h, void* dst, int flags) {
  return get_out(h, &ShepArgs::adj, h ? (size_t)h->a.N * h->a.N : 0, dst, flags);
}

int shep_get_rewards(shep_handle* h, void* dst, int flags) { return get_out(h, &ShepArgs::rew, 1, dst, flags); }

int shep_get_outputs(shep_handle* h, double* dst) {
  return get_out(h, &ShepArgs::obs, h ? (size_t)h->a.N * (4 + h->a.N) + 1 : 0, dst, 0);
}

int shep_get_controls(shep_handle* h, double* dst) {
  if (!h || !dst) return fail(GF_EINVAL, "null argument");
  if (!h->has_ctrl) return fail(GF_ESTATE, "no step yet (shep_step or shep_step_expert first)");
  GF_HIP(hipSetDevice(h->cfg.device));
  return copy_out(h, h->a.ctrl, (size_t)h->a.B * h->a.N * 2, dst, 0);
}

int shep_sync(shep_handle* h) {
  if (!h) return fail(GF_EINVAL, "null handle");
  GF_HIP(hipSetDevice(h->cfg.device));
  GF_HIP(hipStreamSynchronize(h->stream));
  return GF_OK;
}

}  // extern "C"
