// Shepherding-v0: reset() on the device from per-env MT19937 streams (reference
// gym_flock/envs/shepherding/shepherding.py:187-202) and whole recorded expert rollouts
// that run across episode ends in one launch; C-ABI shep_set_rng, shep_get_rng,
// shep_reset_device, shep_expert_rollout, shep_get_episode_steps (include/gymflock.h).
//
// The launch shapes are shep_kernel's (shepherd.hip): one wave per env for N <= 64, four
// envs per workgroup; one workgroup per env above. The per-step arithmetic is
// shepherd_internal.h's, the same code shep_kernel compiles.
//
// A reset takes 4N words of the env's stream: N doubles for the lengths, then N for the
// angles (:193-194), each double NumPy's random_sample of two consecutive words. The env's
// key lives in LDS (624 words); a regeneration runs on it through mt_regen, by the env's
// wave alone in the wave shape (WaveSync: the reset contains no workgroup barrier there,
// so the four envs of a workgroup reset independently) and by the first two waves of the
// workgroup in the other. Lengths and angles land in the LDS slots of x and y, then lane i
// turns its own pair into a position with the device's cos / sin.
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
using SyncOf = std::conditional_t<WAVE, gf::WaveSync, gf::WgSync>;

// RandomState(seed): init_genrand into the key in LDS, by one thread
__device__ __forceinline__ void seed_key(uint32_t* key, uint32_t s) {
  for (int p = 0; p < gf::kMtN; ++p) {
    key[p] = s;
    s = 1812433253u * (s ^ (s >> 30)) + static_cast<uint32_t>(p + 1);
  }
}

// The 2N doubles of a reset from the key in LDS at position pos (env-uniform): lengths
// sqrt(0 + r_max d) to len[0..N), angles pi (0 + 2 d) to ang[0..N). tid in [0, G): the
// caller among the env's G threads, all of which call it. The words are taken key block by
// key block: words [done, done + take) of the reset are key[pos ...]; a double whose words
// lie either side of a regeneration carries its first word over it. Ends with a barrier.
template <bool WAVE>
__device__ __forceinline__ void reset_draw(uint32_t* key, int& pos, int tid, int G, int N, double r_max, double* len,
                                           double* ang) {
  const SyncOf<WAVE> sync;
  constexpr int RT = WAVE ? 64 : 128;  // threads that regenerate (a workgroup here has >= 128)
  const int rtid = tid < RT ? tid : gf::kMtN;
  auto emit = [&](int d, uint32_t wa, uint32_t wb) {
    const double u = (static_cast<double>(wa >> 5) * 67108864.0 + static_cast<double>(wb >> 6)) / 9007199254740992.0;
    if (d < N)
      len[d] = sqrt(0.0 + r_max * u);
    else
      ang[d - N] = M_PI * (0.0 + 2.0 * u);
  };
  const int W = 4 * N;
  int done = 0;
  uint32_t carry = 0;
  while (done < W) {
    if (pos == gf::kMtN) {
      gf::mt_regen<RT, SyncOf<WAVE>>(key, rtid);  // its first barrier orders the reads below before its writes
      pos = 0;
    }
    const int take = min(gf::kMtN - pos, W - done);
    const int off = pos - done;  // word k of the reset is key[off + k]
    if ((done & 1) && tid == 0) emit(done >> 1, carry, gf::mt_temper(key[pos]));
    const int dend = (done + take) >> 1;
    for (int d = ((done + 1) >> 1) + tid; d < dend; d += G)
      emit(d, gf::mt_temper(key[off + 2 * d]), gf::mt_temper(key[off + 2 * d + 1]));
    if ((done + take) & 1) carry = gf::mt_temper(key[pos + take - 1]);
    done += take;
    pos += take;
  }
  sync();
}

// reset() :193-200 of the env in LDS from its key in LDS: new x, y in the lane's registers
// and in LDS, the heading kept. Every thread of the env calls it. Ends with a barrier.
template <bool WAVE>
__device__ __forceinline__ void reset_env(const ShepArgs& a, const ShepRollArgs& r, const Lane<WAVE>& l, uint32_t* key,
                                          int& pos, double& xi, double& yi) {
  const SyncOf<WAVE> sync;
  reset_draw<WAVE>(key, pos, l.i, l.G, a.N, r.r_max, l.sx, l.sy);
  if (l.valid) {  // lane i alone reads and writes slot i
    const double len = l.sx[l.i], ang = l.sy[l.i];
    xi = len * cos(ang);
    yi = len * sin(ang);
    xi = xi + r.off0;
    yi = yi + r.off1;
    l.sx[l.i] = xi;
    l.sy[l.i] = yi;
  }
  sync();
}

template <bool WAVE>
__device__ __forceinline__ void load_key(const ShepRollArgs& r, const Lane<WAVE>& l, uint32_t* key, int& pos) {
  for (int k = l.i; k < gf::kMtN; k += l.G) key[k] = r.mt_key[(size_t)l.b * gf::kMtN + k];
  const int p = min(max(r.mt_pos[l.b], 0), gf::kMtN);
  pos = WAVE ? __builtin_amdgcn_readfirstlane(p) : p;
}

template <bool WAVE>
__device__ __forceinline__ void store_key(const ShepRollArgs& r, const Lane<WAVE>& l, const uint32_t* key, int pos) {
  for (int k = l.i; k < gf::kMtN; k += l.G) r.mt_key[(size_t)l.b * gf::kMtN + k] = key[k];
  if (l.i == 0) r.mt_pos[l.b] = pos;
}

// the tail of shep_kernel: reward, observation, state and adjacency of the state in LDS
template <bool WAVE>
__device__ __forceinline__ void write_tail(const ShepArgs& a, const Lane<WAVE>& l, double xi, double yi, double ti) {
  const int i = l.i, N = a.N;
  const double rw = reward_of<WAVE>(a, l, xi, yi);
  if (l.active && i == 0) a.rew[l.b] = rw;
  if (l.valid) {
    write_obs(a.obs + ((size_t)l.b * N + i) * 4, i, a.nsh, xi, yi, ti);
    double* p = a.x + ((size_t)l.b * N + i) * 3;
    p[0] = xi;
    p[1] = yi;
    p[2] = ti;
    write_adj(a.adj + (size_t)l.b * N * N, a, i, l.sx, l.sy, xi, yi);
  }
}

// shep_reset_device: the selected envs' reset, then their observation as shep_observe
// writes it. Unselected envs are not touched. No workgroup barrier in the wave shape.
template <bool WAVE>
__global__ __launch_bounds__(WAVE ? 64 * kWaveEnvs : kMaxAgents) void shep_reset_kernel(ShepArgs a, ShepRollArgs r) {
  constexpr int S = Lane<WAVE>::S;
  __shared__ double s_state[(WAVE ? kWaveEnvs : 1) * 3 * S];
  __shared__ uint32_t s_key[(WAVE ? kWaveEnvs : 1) * gf::kMtN];
  const SyncOf<WAVE> sync;
  const Lane<WAVE> l(a, s_state, nullptr);
  if (!l.active || (r.mask && !r.mask[l.b])) return;  // uniform over the env's threads
  const int i = l.i;
  uint32_t* key = s_key + l.e * gf::kMtN;
  double xi = 0, yi = 0, ti = 0;
  if (l.valid) {
    ti = r.zero_headings ? 0.0 : a.x[((size_t)l.b * a.N + i) * 3 + 2];
    l.sth[i] = ti;
  }
  int pos = gf::kMtN;
  if (r.seeded) {
    if (i == 0) seed_key(key, r.seed0 + static_cast<uint32_t>(l.b));
  } else {
    load_key<WAVE>(r, l, key, pos);
  }
  sync();
  reset_env<WAVE>(a, r, l, key, pos, xi, yi);
  store_key<WAVE>(r, l, key, pos);
  write_tail<WAVE>(a, l, xi, yi, ti);
}

// shep_expert_rollout: n_steps of u = controller(); step(u) with the state in LDS, as
// shep_kernel's rollout mode, recording on the way; with L > 0 an env whose episode step
// count reaches L is reset from its own stream right after that step.
template <bool WAVE>
__global__ __launch_bounds__(WAVE ? 64 * kWaveEnvs : kMaxAgents) void shep_rollout_kernel(ShepArgs a, ShepRollArgs r) {
  constexpr int S = Lane<WAVE>::S;
  __shared__ double s_state[(WAVE ? kWaveEnvs : 1) * 3 * S];
  __shared__ int s_flag[(WAVE ? kWaveEnvs : 1) * S];
  __shared__ uint32_t s_key[(WAVE ? kWaveEnvs : 1) * gf::kMtN];
  const Lane<WAVE> l(a, s_state, s_flag);
  const int i = l.i;
  const int64_t b = l.b;
  const int N = a.N, nsh = a.nsh, B = a.B;
  const bool active = l.active, valid = l.valid;
  double *sx = l.sx, *sy = l.sy, *sth = l.sth;
  uint32_t* key = s_key + l.e * gf::kMtN;

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
  int cnt = 0, pos = 0, nres = 0;  // env-uniform
  if (r.L > 0 && active) {
    load_key<WAVE>(r, l, key, pos);
    const int c0 = r.count0[b];
    cnt = WAVE ? __builtin_amdgcn_readfirstlane(c0) : c0;
  }
  __syncthreads();

  int since = 0;
  size_t row = 0;  // the next recorded row
  for (int t = 0; t < r.n_steps; ++t) {
    double c = 0, s = 0, ux = 0, uy = 0;
    if (valid) {
      c = cos(ti);
      s = sin(ti);
    }
    double vx = 0, vy = 0;
    controller_out<WAVE>(a, l, xi, yi, ti, c, s, vx, vy);
    if (valid && i < nsh) {
      if (r.actions) {
        const size_t o = (((size_t)t * B + b) * nsh + i) * 2;
        if (r.f32) {
          float* d = static_cast<float*>(r.actions) + o;
          d[0] = (float)vx;
          d[1] = (float)vy;
        } else {
          double* d = static_cast<double*>(r.actions) + o;
          d[0] = vx;
          d[1] = vy;
        }
      }
      ux = vx * a.action_scalar;
      uy = vy * a.action_scalar;
    }
    if (valid && i >= nsh) sheep_sum(a, i, sx, sy, xi, yi, ux, uy);
    if (valid) {
      unicycle(a, i >= nsh, c, s, ux, uy, xi, yi, ti);
      if (t == r.n_steps - 1) {
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
    if (r.rewards) {
      const double rw = reward_of<WAVE>(a, l, xi, yi);
      if (active && i == 0) r.rewards[(size_t)t * B + b] = rw;
    }
    ++cnt;
    const bool done = r.L > 0 && cnt >= r.L;
    if (r.done && active && i == 0) r.done[(size_t)t * B + b] = done ? 1 : 0;
    if (done && active) {  // uniform over the env's threads; the workgroup's in its shape
      reset_env<WAVE>(a, r, l, key, pos, xi, yi);
      cnt = 0;
      ++nres;
    }
    if (++since == r.every) {
      since = 0;
      if (valid) {
        if (r.obs) {
          const size_t o = ((row * B + b) * N + i) * 4;
          if (r.f32)
            write_obs(static_cast<float*>(r.obs) + o, i, nsh, xi, yi, ti);
          else
            write_obs(static_cast<double*>(r.obs) + o, i, nsh, xi, yi, ti);
        }
        if (r.adj) {
          const size_t o = (row * B + b) * N * N;
          if (r.f32)
            write_adj(static_cast<float*>(r.adj) + o, a, i, sx, sy, xi, yi);
          else
            write_adj(static_cast<double*>(r.adj) + o, a, i, sx, sy, xi, yi);
        }
      }
      ++row;
    }
  }
  if (active) {
    if (nres > 0) store_key<WAVE>(r, l, key, pos);
    if (r.n_resets && i == 0) r.n_resets[b] = nres;
  }
  write_tail<WAVE>(a, l, xi, yi, ti);
}

int ensure_rng(shep_handle* h) {
  if (h->mt_key) return GF_OK;
  const size_t B = (size_t)h->a.B;
  if (int rc = dalloc(&h->mt_key, B * gf::kMtN)) return rc;
  if (int rc = dalloc(&h->mt_pos, B)) return rc;
  return GF_OK;
}

int check_reset_config(const shep_reset_config* rc) {
  if (!rc) return fail(GF_EINVAL, "null reset config");
  if (!std::isfinite(rc->r_max) || !(rc->r_max > 0)) return fail(GF_EINVAL, "r_max must be finite and > 0");
  if (!std::isfinite(rc->goal_offset[0]) || !std::isfinite(rc->goal_offset[1]))
    return fail(GF_EINVAL, "goal_offset must be finite");
  return GF_OK;
}

template <class K>
int launch_shape(shep_handle* h, K wave, K wg, const ShepArgs& a, const ShepRollArgs& r, const char* what) {
  if (a.N <= 64) {
    const unsigned grid = (unsigned)((a.B + kWaveEnvs - 1) / kWaveEnvs);
    hipLaunchKernelGGL(wave, dim3(grid), dim3(64 * kWaveEnvs), 0, h->stream, a, r);
  } else {
    hipLaunchKernelGGL(wg, dim3((unsigned)a.B), dim3((unsigned)((a.N + 63) / 64 * 64)), 0, h->stream, a, r);
  }
  GF_LAUNCH(what, hipGetLastError());
  return GF_OK;
}

// the episode step count after n steps from c with in-launch resets at L (L > 0)
int32_t count_after(int32_t c, int n, int L) {
  const int64_t first = std::max<int64_t>(1, (int64_t)L - c);  // the steps up to the first done one
  if (n < first) return c + n;
  return (int32_t)((n - first) % L);
}

size_t align16(size_t n) { return (n + 15) / 16 * 16; }

}  // namespace

extern "C" {

int shep_set_rng(shep_handle* h, int env, const uint32_t* keys, const int32_t* pos) {
  if (!h || !keys || !pos || env < -1) return fail(GF_EINVAL, "bad argument");
  if (env >= h->a.B) return fail(GF_EINVAL, "env out of range");
  const size_t n = env < 0 ? (size_t)h->a.B : 1, first = env < 0 ? 0 : (size_t)env;
  for (size_t k = 0; k < n; ++k)
    if (pos[k] < 0 || pos[k] > gf::kMtN) return fail(GF_EINVAL, "stream position outside [0, 624]");
  GF_HIP(hipSetDevice(h->cfg.device));
  if (int rc = ensure_rng(h)) return rc;
  GF_HIP(hipMemcpyAsync(h->mt_key + first * gf::kMtN, keys, n * gf::kMtN * sizeof(uint32_t), hipMemcpyHostToDevice,
                        h->stream));
  GF_HIP(hipMemcpyAsync(h->mt_pos + first, pos, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  for (size_t k = 0; k < n; ++k) h->rng_set[first + k] = 1;
  return GF_OK;
}

int shep_get_rng(shep_handle* h, int env, uint32_t* keys, int32_t* pos) {
  if (!h || !keys || !pos || env < -1) return fail(GF_EINVAL, "bad argument");
  if (env >= h->a.B) return fail(GF_EINVAL, "env out of range");
  const size_t n = env < 0 ? (size_t)h->a.B : 1, first = env < 0 ? 0 : (size_t)env;
  for (size_t k = 0; k < n; ++k)
    if (!h->rng_set[first + k])
      return fail(GF_ESTATE, "shep_get_rng: the env's stream was never seeded or set (shep_reset_device, shep_set_rng)");
  GF_HIP(hipSetDevice(h->cfg.device));
  GF_HIP(hipMemcpyAsync(keys, h->mt_key + first * gf::kMtN, n * gf::kMtN * sizeof(uint32_t), hipMemcpyDeviceToHost,
                        h->stream));
  GF_HIP(hipMemcpyAsync(pos, h->mt_pos + first, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  return GF_OK;
}

int shep_reset_device(shep_handle* h, const shep_reset_config* rc, uint64_t seed, const uint8_t* env_mask, int flags) {
  if (!h || !rc) return fail(GF_EINVAL, "null argument");
  if (flags & ~(SHEP_RESET_SEED | SHEP_RESET_ZERO_HEADINGS)) return fail(GF_EINVAL, "shep_reset_device: unknown flag");
  if (int r = check_reset_config(rc)) return r;
  const int B = h->a.B;
  const bool seeded = flags & SHEP_RESET_SEED;
  if (seeded && (seed > 0xffffffffull || seed + (uint64_t)B > 0x100000000ull))
    return fail(GF_EINVAL, "seed + n_envs must fit in 32 bits");
  int n_sel = B;
  if (env_mask) {
    n_sel = 0;
    for (int b = 0; b < B; ++b) n_sel += env_mask[b] ? 1 : 0;
    if (n_sel == 0) return GF_OK;
  }
  if (!seeded)
    for (int b = 0; b < B; ++b)
      if ((!env_mask || env_mask[b]) && !h->rng_set[b])
        return fail(GF_ESTATE,
                    "shep_reset_device: a selected env's stream was never seeded or set (SHEP_RESET_SEED or shep_set_rng)");
  GF_HIP(hipSetDevice(h->cfg.device));
  if (int r = ensure_rng(h)) return r;
  const bool partial = n_sel < B;
  if (!h->has_state) {  // a handle without a state resets as from the all-zero state
    GF_HIP(hipMemsetAsync(h->a.x, 0, sizeof(double) * 3 * B * h->a.N, h->stream));
    h->has_state = true;
    h->has_obs = false;
  }
  if (partial && !h->has_obs)  // the unselected envs' outputs are their states'
    if (int r = shep_observe(h)) return r;
  ShepRollArgs ra{};
  if (partial) {
    if (!h->mask_dev)
      if (int r = dalloc(&h->mask_dev, (size_t)B)) return r;
    // pageable host memory: the copy has left the caller's mask when this returns
    GF_HIP(hipMemcpyAsync(h->mask_dev, env_mask, (size_t)B, hipMemcpyHostToDevice, h->stream));
    ra.mask = h->mask_dev;
  }
  ra.r_max = rc->r_max;
  ra.off0 = rc->goal_offset[0];
  ra.off1 = rc->goal_offset[1];
  ra.mt_key = h->mt_key;
  ra.mt_pos = h->mt_pos;
  ra.seeded = seeded ? 1 : 0;
  ra.seed0 = static_cast<uint32_t>(seed);
  ra.zero_headings = (flags & SHEP_RESET_ZERO_HEADINGS) ? 1 : 0;
  if (int r = launch_shape(h, shep_reset_kernel<true>, shep_reset_kernel<false>, h->a, ra, "shep_reset_kernel")) return r;
  for (int b = 0; b < B; ++b)
    if (!partial || env_mask[b]) {
      h->rng_set[b] = 1;
      h->ep_count[b] = 0;
    }
  h->has_obs = true;
  h->has_ctrl = false;
  return GF_OK;
}

int shep_get_episode_steps(shep_handle* h, int32_t* out) {
  if (!h || !out) return fail(GF_EINVAL, "null argument");
  std::copy(h->ep_count.begin(), h->ep_count.end(), out);
  return GF_OK;
}

int shep_expert_rollout(shep_handle* h, int n_steps, int record_every, int episode_length, const shep_reset_config* rc,
                        const shep_rollout_records* rec, int flags) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (flags & ~(SHEP_REC_DEVICE | SHEP_REC_F32)) return fail(GF_EINVAL, "shep_expert_rollout: unknown flag");
  if (n_steps < 1) return fail(GF_EINVAL, "n_steps must be >= 1");
  if (record_every < 1 || n_steps % record_every) return fail(GF_EINVAL, "record_every must be >= 1 and divide n_steps");
  if (episode_length < 0) return fail(GF_EINVAL, "episode_length must be >= 0");
  if (episode_length > 0)
    if (int r = check_reset_config(rc)) return r;
  if (!h->has_state) return fail(GF_ESTATE, "set a state first (shep_set_state or shep_reset_device)");
  const int B = h->a.B, N = h->a.N, nsh = h->a.nsh;
  if (episode_length > 0)
    for (int b = 0; b < B; ++b)
      if (!h->rng_set[b])
        return fail(GF_ESTATE, "shep_expert_rollout: an env's stream was never seeded or set (shep_reset_device with "
                               "SHEP_RESET_SEED, or shep_set_rng)");
  GF_HIP(hipSetDevice(h->cfg.device));
  const bool dev = flags & SHEP_REC_DEVICE, f32 = flags & SHEP_REC_F32;
  const size_t K = (size_t)(n_steps / record_every), T = (size_t)n_steps, el = f32 ? 4 : 8;
  const shep_rollout_records none{};
  const shep_rollout_records& q = rec ? *rec : none;
  // the records' sizes in bytes, in the order of the struct
  void* const host[6] = {q.obs, q.adj, q.actions, q.rewards, q.done, q.n_resets};
  const size_t bytes[6] = {K * B * N * 4 * el, K * B * N * N * el, T * B * nsh * 2 * el,
                           T * B * sizeof(double), T * B, (size_t)B * sizeof(int32_t)};
  void* dst[6];
  bool any = false;
  for (int k = 0; k < 6; ++k) {
    dst[k] = host[k];
    any = any || host[k];
  }
  if (!dev && any) {  // the records pass through device memory of the handle's
    size_t total = 0;
    for (int k = 0; k < 6; ++k)
      if (host[k]) total += align16(bytes[k]);
    if (h->rec_cap < total) {
      GF_HIP(hipStreamSynchronize(h->stream));
      if (h->rec) GF_HIP(hipFree(h->rec));
      h->rec = nullptr;
      h->rec_cap = 0;
      if (int r = dalloc(&h->rec, total)) return r;
      h->rec_cap = total;
    }
    size_t at = 0;
    for (int k = 0; k < 6; ++k)
      if (host[k]) {
        dst[k] = h->rec + at;
        at += align16(bytes[k]);
      }
  }
  ShepRollArgs ra{};
  ra.n_steps = n_steps;
  ra.every = record_every;
  ra.L = episode_length;
  ra.f32 = f32 ? 1 : 0;
  ra.obs = dst[0];
  ra.adj = dst[1];
  ra.actions = dst[2];
  ra.rewards = static_cast<double*>(dst[3]);
  ra.done = static_cast<uint8_t*>(dst[4]);
  ra.n_resets = static_cast<int32_t*>(dst[5]);
  if (episode_length > 0) {
    if (!h->count_dev)
      if (int r = dalloc(&h->count_dev, (size_t)B)) return r;
    // pageable host memory: the copy has left ep_count when this returns
    GF_HIP(hipMemcpyAsync(h->count_dev, h->ep_count.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice,
                          h->stream));
    ra.count0 = h->count_dev;
    ra.mt_key = h->mt_key;
    ra.mt_pos = h->mt_pos;
    ra.r_max = rc->r_max;
    ra.off0 = rc->goal_offset[0];
    ra.off1 = rc->goal_offset[1];
  }
  if (int r = launch_shape(h, shep_rollout_kernel<true>, shep_rollout_kernel<false>, h->a, ra, "shep_rollout_kernel"))
    return r;
  if (episode_length > 0)
    for (int32_t& c : h->ep_count) c = count_after(c, n_steps, episode_length);
  else
    h->count_steps(n_steps);
  h->has_obs = h->has_ctrl = true;
  if (!dev && any) {
    for (int k = 0; k < 6; ++k)
      if (host[k]) GF_HIP(hipMemcpyAsync(host[k], dst[k], bytes[k], hipMemcpyDeviceToHost, h->stream));
    GF_HIP(hipStreamSynchronize(h->stream));
  }
  return GF_OK;
}

}  // extern "C"
