// The double-integrator update of one agent, shared by the step kernels
// (flock_kernels.hip) and the closed-loop rollout (flock_rollout.hip): the arithmetic
// only, on values the caller has already loaded, in the reference's operation order.
// Both translation units are built with -ffp-contract=off, so both round alike.
#pragma once
#include <type_traits>

#include "flock_internal.h"

namespace gf {

struct __attribute__((aligned(16))) St {
  double px, py, vx, vy;
};

template <class V>
__device__ __forceinline__ V clip_sym(V v, V c) {  // np.clip(v, -c, c); NaN stays NaN
  return v < -c ? -c : (v > c ? c : v);
}

__device__ __forceinline__ double clip10(double v) {  // np.clip(v, -10, 10); NaN stays NaN
  return v < -10.0 ? -10.0 : (v > 10.0 ? 10.0 : v);
}

template <bool UF64>
using ActionT = typename std::conditional<UF64, double2, float2>::type;

// State of an agent after the double-integrator update of flocking_relative.py:96-105, in
// the reference's operation order. With a float32 u the action terms are float32
// arithmetic (NumPy keeps u*10.0, *dt, *0.5 in float32) and are widened when added to the
// float64 state.
template <bool UF64>
__device__ __forceinline__ St integrate_plain(const StepArgs& a, double2 p, double2 v, ActionT<UF64> u) {
  St s{p.x, p.y, v.x, v.y};
  if constexpr (UF64) {
    const double ux = u.x * a.action_scalar, uy = u.y * a.action_scalar;
    s.px = (p.x + v.x * a.dt) + ((ux * a.dt) * a.dt) * 0.5;
    s.py = (p.y + v.y * a.dt) + ((uy * a.dt) * a.dt) * 0.5;
    s.vx = v.x + ux * a.dt;
    s.vy = v.y + uy * a.dt;
  } else {
    const float ux = u.x * a.as_f, uy = u.y * a.as_f;
    const float apx = ((ux * a.dt_f) * a.dt_f) * 0.5f;
    const float apy = ((uy * a.dt_f) * a.dt_f) * 0.5f;
    s.px = (p.x + v.x * a.dt) + static_cast<double>(apx);
    s.py = (p.y + v.y * a.dt) + static_cast<double>(apy);
    s.vx = v.x + static_cast<double>(ux * a.dt_f);
    s.vy = v.y + static_cast<double>(uy * a.dt_f);
  }
  return s;
}

// The variants' update (oracle/flocking_variants.integrate) of agent j of an env whose
// step is dt: optional clip, the step's own action scale, the frozen agents' float64 mask
// applied after the action arithmetic, and the stochastic env's state scaling around the
// update.
template <bool UF64>
__device__ __forceinline__ St integrate_variant(const StepArgs& a, double dt, int j, double2 p, double2 v,
                                                ActionT<UF64> u) {
  const double m = j < a.n_frozen ? 0.0 : 1.0;
  const double S = a.x_scale;
  const double px = p.x * S, py = p.y * S, vx = v.x * S, vy = v.y * S;
  double apx, apy, avx, avy;
  if constexpr (UF64) {
    double ux = u.x, uy = u.y;
    if (a.u_clip > 0) {
      ux = clip_sym(ux, a.u_clip);
      uy = clip_sym(uy, a.u_clip);
    }
    ux *= a.u_scale;
    uy *= a.u_scale;
    apx = (((ux * dt) * dt) * 0.5) * m;
    apy = (((uy * dt) * dt) * 0.5) * m;
    avx = (ux * dt) * m;
    avy = (uy * dt) * m;
  } else {
    const float dtf = static_cast<float>(dt);
    float ux = u.x, uy = u.y;
    if (a.u_clip > 0) {
      ux = clip_sym(ux, a.uc_f);
      uy = clip_sym(uy, a.uc_f);
    }
    ux *= a.us_f;
    uy *= a.us_f;
    apx = static_cast<double>(((ux * dtf) * dtf) * 0.5f) * m;
    apy = static_cast<double>(((uy * dtf) * dtf) * 0.5f) * m;
    avx = static_cast<double>(ux * dtf) * m;
    avy = static_cast<double>(uy * dtf) * m;
  }
  St s;
  s.px = ((px + vx * dt) + apx) / S;
  s.py = ((py + vy * dt) + apy) / S;
  s.vx = (vx + avx) / S;
  s.vy = (vy + avy) / S;
  return s;
}

}  // namespace gf
