/*
 * gymflock.h — C-ABI of libgymflock.so, the MI355X (gfx950) env-step engine for
 * gym-flock's FlockingRelative-v0 / Flocking-v0 hot path.
 *
 * The reference (katetolstaya/gym-flock) has no FFI: its boundary is the Python
 * gym.Env method surface. Each entry point below replaces one
 * NumPy code region of that surface; the citation after each declaration names it
 * (paths relative to the reference root). The Python binding that sits on top of
 * this ABI (gym-flock_amd/gym_flock/_native.py, ctypes) mirrors the reference's
 * reset()/step()/controller()/get_stats() methods; INTEGRATION.md shows it.
 *
 * Conventions
 *  - Every function returns int: GF_OK (0) or a GF_E* code; the message of the
 *    last failure on the calling thread is fe_last_error().
 *  - Arrays are row-major, C-contiguous. Shapes use B = n_envs, N = n_agents.
 *  - Host pointers are borrowed for the duration of the call. The library owns
 *    all device memory; fe_device_buffers() exposes it for zero-copy consumers.
 *  - One handle per host thread. A step's two half-batch launches run on the
 *    handle's stream and a second one (fe_set_streams); every other call orders the
 *    handle's stream after both first, and getters synchronise it before copying out.
 *    Zero-copy consumers of fe_buffers.stream call fe_join() after fe_step.
 *  - Agent state is float64 (B,N,4) = [px, py, vx, vy] because the reference
 *    integrates in float64 (flocking_relative.py:157); observations are float32.
 */
#ifndef GYMFLOCK_H
#define GYMFLOCK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GF_ABI_VERSION 1

enum gf_status {
  GF_OK = 0,
  GF_EINVAL = 1,   /* bad argument (shape, pointer, flag)                      */
  GF_EHIP = 2,     /* HIP runtime error (no device, launch failure, ...)       */
  GF_ENOMEM = 3,   /* device allocation failed                                  */
  GF_ESTATE = 4,   /* call out of order (e.g. step before set_state)            */
  GF_ECOMM = 5     /* RCCL error                                                */
};

/* fe_step / fe_compute_helpers flags */
#define FE_WITH_CONTROLLER 0x01 /* also run controller() on the post-step state   */
#define FE_U_DEVICE        0x02 /* u is a device pointer (else host)              */
#define FE_U_F64           0x04 /* u is float64 (else float32); selects the NumPy
                                   dtype-dependent arithmetic of :96-105          */
#define FE_U_EXPERT        0x08 /* u := controller output of the previous call
                                   (closed loop, float64; u argument ignored)     */
#define FE_WITH_KNN        0x10 /* Flocking-v0 k-nearest observation              */
#define FE_NO_NETWORK      0x20 /* skip the dense (N,N) state_network write       */
#define FE_NO_STATE_VALUES 0x40 /* skip the (N,6) state_values write              */
#define FE_U_RESIDENT      0x80 /* u := the handle's action buffer as last set by
                                   fe_set_actions (already in HBM; u ignored)     */
#define FE_OUT_MAPPED        0x1 /* fe_get_outputs: destinations that are page-locked
                                   (fe_host_alloc) are written by one device copy
                                   kernel through their mapped addresses instead of
                                   one DMA copy each; others still take a copy     */
#define FE_PACKED_NETWORK 0x100 /* also write the adjacency as bits (B,N,ceil(N/64))
                                   uint64 + degree (B,N) int32, the packed output
                                   mode; with FE_NO_NETWORK the
                                   dense (N,N) write is skipped: 32x fewer bytes  */

typedef struct fe_config {
  int32_t n_agents;      /* N  (flocking_relative.py:38; params_from_cfg :74)      */
  int32_t n_envs;        /* B  independent envs batched on this device            */
  double comm_radius;    /* 0.9  (:39)                                            */
  double dt;             /* 0.01 (:40)                                            */
  double action_scalar;  /* 10.0 (:64)                                            */
  int32_t mean_pooling;  /* 1 (:27): network = adj / deg, else adj                */
  int32_t centralized;   /* 1 (:28): controller sums over all agents              */
  int32_t n_neighbors;   /* k of Flocking-v0 (flocking.py:9, 7); 0 = no kNN buffers */
  int32_t device;        /* HIP device ordinal                                    */
} fe_config;

typedef struct fe_handle fe_handle;

/* Flocking variants on the same step. Defaults reproduce
 * FlockingRelative-v0; the registered variants set (reference files under
 * gym_flock/envs/flocking/):
 *   FlockingLeader-v0      u_scale 1, n_frozen 2               (flocking_leader.py:13-15, :21-33)
 *   FlockingObstacle-v0    u_scale 1, n_frozen 4, n_vel_zero 4 (flocking_obstacle.py:19-21, :34-49, :75-80)
 *   FlockingStochastic-v0  u_scale 6, u_clip 0.5, x_scale 6, ctrl_clip 0.5, per-step dt
 *                          (flocking_stoch.py:9-12, :14-36, :39-46; dt via fe_set_dt)
 *   FlockingTwoFlocks-v0   defaults (only its reset differs, host side)        */
typedef struct fe_variant {
  int32_t n_frozen;      /* agents [0,n) ignore actions: their mask is 0 (leaders, obstacles) */
  int32_t n_vel_zero;    /* pairs touching agents [0,n) have zero velocity difference          */
  double u_scale;        /* the step's action multiplier (10 = cfg action_scalar by default);
                            the controller still divides by cfg action_scalar (:211)          */
  double u_clip;         /* clip actions to +-u_clip before scaling; <= 0: none               */
  double x_scale;        /* state multiplied before and divided after the update; 1: none     */
  double ctrl_clip;      /* controller output clip after the /action_scalar; <= 0: none       */
} fe_variant;

/* Device pointers owned by the handle (valid until fe_destroy). Ping-pong
 * buffers are reported as their CURRENT slot (the one the next getter reads).
 * state_values and network are NULL while the last observation went to host arrays
 * only (fe_step_host / fe_step_host_knn*: the device copies are stale then). */
typedef struct fe_buffers {
  double* x;             /* (B,N,4) float64 current state                        */
  float* state_values;   /* (B,N,6) float32                                      */
  float* network;        /* (B,N,N) float32                                      */
  double* controls;      /* (B,N,2) float64 last controller() output             */
  double* rewards;       /* (B)     float64                                      */
  int32_t* knn_idx;      /* (B,N,k) int32 or NULL                                */
  float* knn_obs;        /* (B,N,4k) float32 or NULL                             */
  void* stream;          /* hipStream_t of the handle                            */
  uint64_t* adj_bits;    /* (B,N,ceil(N/64)) packed adjacency or NULL (FE_PACKED_NETWORK) */
  int32_t* degree;       /* (B,N) neighbour counts or NULL (FE_PACKED_NETWORK)   */
} fe_buffers;

/* Lifecycle ---------------------------------------------------------------- */
int fe_create(const fe_config* cfg, fe_handle** out);      /* FlockingRelativeEnv.__init__ :20-66 */
int fe_destroy(fe_handle* h);                               /* close() :303 */
int fe_get_config(const fe_handle* h, fe_config* out);
/* Change comm_radius, dt, action_scalar, mean_pooling and centralized for the following
 * launches, keeping the state (the reference reads these attributes at call time, e.g.
 * self.centralized in controller() :200-201). n_agents, n_envs, n_neighbors and device
 * must equal the handle's (GF_EINVAL otherwise). A change of comm_radius, centralized or
 * action_scalar drops the last controller output (it was computed under the old values):
 * FE_U_EXPERT and fe_get_controls then need a new fe_controller / FE_WITH_CONTROLLER. */
int fe_set_params(fe_handle* h, const fe_config* cfg);

/* State ---------------------------------------------------------------------- */
int fe_set_state(fe_handle* h, const double* x);            /* env.x = ... (:189) */
int fe_set_state_env(fe_handle* h, int env, const double* x);  /* one env's (N,4) */
/* Synthetic init (reset()'s distribution without the rejection loop,
 * :164-175): env b is drawn from MT19937 seeded with seed + b in NumPy
 * RandomState's order (length, angle, bias, vx, vy), with r_max = sqrt(N). The
 * uniforms are NumPy's bit for bit; cos/sin come from the C library, so positions
 * may differ from NumPy's in the last ulp. */
int fe_reset_synthetic(fe_handle* h, uint64_t seed, double v_max);
int fe_get_state(fe_handle* h, double* x);                  /* env.x (B,N,4) */
int fe_get_state_env(fe_handle* h, int env, double* x);     /* one env's (N,4) */

/* reset() on the device (flocking_relative.py:156-192): the rejection sampler of every
 * selected env in one launch, one workgroup per env, each drawing from its env's own
 * MT19937 stream (numpy's legacy RandomState) in the reference's order: length[N],
 * angle[N], bias[2], vx[N], vy[N], 4N+2 doubles per candidate whether it is accepted or
 * not. The uniforms, lengths, angles and velocities are NumPy's bit for bit; positions
 * use the device's double cos / sin (relative difference below 2e-15). A candidate is
 * accepted as :176-184 decide: min over i != j of a_ij = dx*dx + dy*dy has sqrt >=
 * min_dist, and every agent has at least min_degree others with a_ij < comm_radius *
 * comm_radius (the handle's comm_radius, the product rounded on the host). */
typedef struct fe_reset_config {
  double r_max, v_max, v_bias;   /* :167-174; r_max is the reference's self.r_max (sqrt(N) after params_from_cfg) */
  double min_dist;               /* 0.1 (:160) */
  int32_t min_degree;            /* 2   (:164) */
  int32_t max_tries;             /* 1..65536 */
} fe_reset_config;
#define FE_RESET_SEED      0x1   /* seed env b's stream as RandomState(seed + b) first; else continue it */
#define FE_RESET_NO_REJECT 0x2   /* keep the first draw (the synthetic init) */
#define FE_RESET_EXHAUSTED 0x1   /* status bit: no try was accepted, the last one kept */
/* env_mask: (B) bytes, nonzero = reset this env, or NULL = all; the other envs keep their
 * state, stream, tries and status (a mask selecting none: nothing happens, GF_OK). tries
 * and status: (B) host arrays or NULL. With both NULL the call only enqueues the launch on
 * the handle's stream (after both halves of the latest step); otherwise it waits and
 * copies. An env whose max_tries candidates were all rejected keeps the last one
 * (FE_RESET_EXHAUSTED in its status); its stream stands after max_tries candidates.
 * Afterwards the handle is as after fe_set_state_env: the caller runs fe_compute_helpers
 * (reset() :191). The rejection mode holds a candidate in LDS: n_agents <= 1024 (nothing
 * above roughly 150 agents is ever accepted), GF_EINVAL beyond; FE_RESET_NO_REJECT takes
 * any n_agents. GF_ESTATE without FE_RESET_SEED for an env whose stream was never seeded
 * or set; GF_EINVAL unless seed + n_envs fits in 32 bits. The stream buffers are allocated
 * by the first fe_reset_device / fe_set_rng call of a handle. */
int fe_reset_device(fe_handle* h, const fe_reset_config* rc, uint64_t seed, const uint8_t* env_mask /* (B) or NULL = all */,
                    int flags, int32_t* tries /* (B) host or NULL */, uint8_t* status /* (B) host or NULL */);
/* The envs' streams as RandomState.get_state() has them: keys (624 words each) and
 * positions in [0, 624]. env = -1: all envs, keys (B,624) and pos (B); else one env's. */
int fe_set_rng(fe_handle* h, int env /* -1 = all */, const uint32_t* keys /* (.,624) */, const int32_t* pos);
int fe_get_rng(fe_handle* h, int env, uint32_t* keys, int32_t* pos);
/* The rest of RandomState.get_state(): the Gaussian that legacy_gauss drew with the last
 * one and has not handed out yet (has_gauss 0 or 1, and its value). Only the dt draws of
 * fe_set_dt_noise use it. fe_set_rng and a reset with FE_RESET_SEED clear it for the envs
 * they touch, as RandomState.set_state with a 3-tuple and a fresh RandomState(seed) do; a
 * continued reset leaves it alone (uniform does not touch it). env = -1: all envs, (B)
 * each; else one env's. fe_get_rng_gauss: GF_ESTATE for a stream never seeded or set. */
int fe_set_rng_gauss(fe_handle* h, int env /* -1 = all */, const int32_t* has_gauss, const double* gauss);
int fe_get_rng_gauss(fe_handle* h, int env, int32_t* has_gauss, double* gauss);

/* The variants' resets on the device, from the same per-env streams, one wave per selected
 * env. env_mask, seed, flags, tries and status work as in fe_reset_device; afterwards the
 * handle is as after fe_set_state_env of the new state.
 *  FE_VRESET_LEADER (flocking_leader.py:37-41): fe_reset_device's launch (rc, FE_RESET_SEED,
 *    FE_RESET_NO_REJECT as there), then one more random_sample u per selected env from the
 *    same stream: w = -v_max + (v_max - -v_max) * u becomes both velocity components of
 *    agents [0, n_special) (0 <= n_special <= n_agents). The reference computes its reset
 *    observation and the first controller output from the state BEFORE that override; this
 *    call leaves the overridden state, and fe_compute_helpers / fe_controller after it see
 *    the leaders' new velocities. The quirk stays with the drop-in FlockingLeaderEnv, which
 *    resets on the host.
 *  FE_VRESET_TWOFLOCKS (flocking_twoflocks.py:8-28): two uniforms in [-v_bias/2, v_bias/2)
 *    (rc->v_bias), positions 0.8 * grid(N, side = int(N/10)) with x fastest, velocities
 *    -position + bias. GF_EINVAL unless side >= 1 and side * int(N/side) == N. n_special
 *    and the rest of rc are ignored. tries = 1, status = 0. GF_ESTATE without FE_RESET_SEED
 *    for a stream never seeded or set.
 *  FE_VRESET_OBSTACLE (flocking_obstacle.py:59-74): no draws (FE_RESET_SEED still seeds the
 *    streams). The flock on grid(N, 5) at velocity (0, -7), the n_special == 4 obstacles on
 *    half of grid(4, 2) moved 10 down, at rest. GF_EINVAL unless 5 * int(N/5) == N and
 *    n_special == 4. tries = 1, status = 0.
 * TwoFlocks and Obstacle take FE_RESET_SEED only. */
#define FE_VRESET_LEADER 1
#define FE_VRESET_TWOFLOCKS 2
#define FE_VRESET_OBSTACLE 3
int fe_reset_variant(fe_handle* h, int kind, const fe_reset_config* rc, int n_special, uint64_t seed,
                     const uint8_t* env_mask /* (B) or NULL = all */, int flags, int32_t* tries /* (B) host or NULL */,
                     uint8_t* status /* (B) host or NULL */);

/* Hot path ------------------------------------------------------------------- */
/* Upload (B,N,2) actions (float32, or float64 if f64) into the handle's resident
 * action buffer, used by fe_step(..., FE_U_RESIDENT). */
int fe_set_actions(fe_handle* h, const void* u, int f64);
/* compute_helpers() on the current state (:111-134); used by reset() (:191). */
int fe_compute_helpers(fe_handle* h, int flags);
/* step(u) (:91-109): dynamics (:96-105) + compute_helpers + instant_cost (:145-147),
 * optionally fused controller() (:194-226) and Flocking-v0 kNN (flocking.py:20-25).
 * u: (B,N,2) float32 or float64 (FE_U_F64), host or device (FE_U_DEVICE). Async. */
int fe_step(fe_handle* h, const void* u, int flags);
/* The expert loop `u = env.controller(); env.step(u)` for n_steps steps in ONE launch, with
 * optional recording (expert demonstrations: the reference README's imitation learning).
 * The same as n_steps calls of fe_step(h, NULL, FE_U_EXPERT | FE_WITH_CONTROLLER |
 * FE_PACKED_NETWORK | FE_NO_NETWORK): states, adjacency bits and degrees bit for bit,
 * state_values, controls and rewards up to summation order (every sum runs in a fixed tree:
 * two runs give the same bits, whatever n_steps and record_every are). One workgroup keeps
 * an env's state in LDS across all steps, so n_agents <= 256 (every size at which the
 * reference's reset() ever accepts a draw); GF_EINVAL above: loop over
 * fe_step(FE_U_EXPERT) there. Variants (fe_set_variant) and a per-env dt (fe_set_dt, the
 * same dt for all n_steps; fe_set_dt_noise, a new one every step) apply as in fe_step.
 * rec (or NULL: nothing recorded): where to put step t's record for every t with
 * (t + 1) % record_every == 0, K = n_steps / record_every of them, and every step's reward.
 * Every pointer may be NULL (not recorded). */
typedef struct fe_rollout {
  double*   x;            /* (K,B,N,4)  state after the step                       */
  float*    state_values; /* (K,B,N,6)                                             */
  uint64_t* adj_bits;     /* (K,B,N,ceil(N/64)) layout of fe_get_network_packed    */
  int32_t*  degree;       /* (K,B,N)                                               */
  double*   controls;     /* (K,B,N,2)  controller() of the state after the step   */
  double*   rewards;      /* (n_steps,B) every step's, whatever record_every is    */
  int32_t   record_every; /* >= 1 and divides n_steps                              */
  int32_t   flags;        /* FE_ROLLOUT_DEVICE: the pointers are caller-owned device memory */
} fe_rollout;
#define FE_ROLLOUT_DEVICE 0x1
/* Runs on the handle's stream after both halves of the latest split step. With rec NULL or
 * FE_ROLLOUT_DEVICE the call only enqueues (device destinations are written by the kernel
 * itself, in stream order); with host destinations the records go through a device staging
 * buffer kept on the handle and the call returns when they are in place.
 * GF_ESTATE without a controller output of the current state (fe_controller, or a step
 * with FE_WITH_CONTROLLER), and on a handle with a communicator (the metrics ring holds 64
 * steps). GF_EINVAL for n_steps < 1, record_every < 1 or not dividing n_steps, unknown
 * flags, n_agents > 256.
 * Afterwards the handle is as after fe_set_state with a controller output: the final state
 * and its controls are the handle's, fe_get_rewards returns the last step's rewards,
 * fe_get_state_values and fe_get_network_packed the last step's. The dense network was not
 * written: fe_get_network, fe_get_network_rows and fe_get_outputs (network) return
 * GF_ESTATE until a launch writes it (fe_compute_helpers, a step without FE_NO_NETWORK),
 * and the next plain step stores it in full (as after fe_network_touched). fe_get_knn
 * ranks the final state anew. Closed-loop stepping, or another rollout, goes on without a
 * new fe_controller. */
int fe_step_expert(fe_handle* h, int n_steps, const fe_rollout* rec /* or NULL */);

/* DAgger rollouts (FlockingRelative-v0, n_agents <= 256): fe_step_expert's loop in which a
 * learner drives with probability 1 - beta per step and env, and the expert labels every
 * state the loop reaches.
 *
 * The learner is one network shared by all agents over delayed aggregation features
 * z_t (N, n_taps, 6) float32 (Tolstaya et al., CoRL 2020, in recursive form):
 *   z_t[i,0,:] = state_values_t[i,:]
 *   z_t[i,k,:] = float32((sum over j adjacent to i in state t of double(z_{t-1}[j,k-1,:])) / d_i), k >= 1,
 * d_i = max(degree_t[i], 1) with mean_pooling, else 1; every tap k >= 1 is zero at an
 * episode's start. Taps 1 .. n_taps-1 of the current state are kept on the handle.
 * Network: n_layers linear layers of widths width[0] = 6 * n_taps, ..., width[n_layers] = 2,
 * hidden widths multiples of 4 and at most 64; weight[l] (width[l+1], width[l]) row-major
 * (torch.nn.Linear.weight), bias[l] (width[l+1]); ReLU (x > 0 ? x : 0) after every layer but
 * the last. All of it float32, in one fixed order: the input is z_t[i] flattened (index
 * 6k + f); an output starts from its bias and adds weight[o][i] * x[i] for i ascending,
 * every product and every sum rounded once (no fused multiply-add). clip > 0 (rounded to
 * float32): both outputs clipped to [-clip, clip]. The action applied is double(output). */
#define FE_ACT_RELU 0
typedef struct fe_policy {
  const float* weight[3]; /* host pointers, copied by the call */
  const float* bias[3];
  double  clip;           /* 0: none */
  int32_t n_taps;         /* 1..4 */
  int32_t n_layers;       /* 1..3 */
  int32_t width[4];
  int32_t activation;     /* FE_ACT_RELU */
  int32_t reserved;
} fe_policy;              /* 88 bytes */
/* NULL removes the policy. Either way the taps of all envs are zeroed. */
int fe_set_policy(fe_handle* h, const fe_policy* policy);
/* Zero the taps k >= 1 of the selected envs (env_mask (B), or NULL: all). The taps advance
 * only in fe_step_policy: a caller that resets envs or sets their state calls this for them,
 * as a caller that sets state calls fe_compute_helpers. GF_ESTATE without a policy. */
int fe_reset_aggregation(fe_handle* h, const uint8_t* env_mask);
/* z of the current state: dst (B,N,n_taps,6), or (N,n_taps,6) of env >= 0. */
int fe_get_aggregation(fe_handle* h, int env /* -1 = all */, float* dst);

/* Records of fe_step_policy: fe_rollout's, of the state after the step (K = n_steps /
 * record_every of them), and the loop's own. (agg, controls) of a record is one DAgger
 * pair. Every pointer may be NULL. */
typedef struct fe_policy_rollout {
  double*   x;            /* as fe_rollout */
  float*    state_values;
  uint64_t* adj_bits;
  int32_t*  degree;
  double*   controls;
  float*    agg;          /* (K,B,N,n_taps,6) z of the recorded state                */
  float*    policy;       /* (K,B,N,2) the learner's action for the recorded state   */
  double*   applied;      /* (n_steps,B,N,2) the action each step integrated         */
  uint8_t*  used_expert;  /* (n_steps,B) 1: that step applied the expert's action    */
  double*   rewards;      /* (n_steps,B)                                             */
  int32_t   record_every;
  int32_t   flags;        /* FE_ROLLOUT_DEVICE */
} fe_policy_rollout;      /* 88 bytes */
/* n_steps of: applied = used_expert ? controller() : policy(z); step(applied); then the new
 * state's observation, controller(), z and policy(z). used_expert[t,b] = (u < beta), u one
 * random_sample() double of env b's stream per step (the stream fe_reset_device seeds and
 * continues; all n_steps doubles are drawn by one launch ahead of the rollout; the cached
 * Gaussian is not touched); beta 0 and 1 draw nothing and need no stream.
 * Stream order, staging and the handle's state afterwards are fe_step_expert's; the taps on
 * the handle are the final state's.
 * GF_EINVAL: n_steps < 1, beta outside [0,1] or NaN, record_every < 1 or not dividing
 * n_steps, unknown flags, n_agents > 256, a handle with a variant, a per-env dt or
 * fe_set_dt_noise. GF_ESTATE: no policy, no controller output of the current state,
 * 0 < beta < 1 with a stream never seeded or set, a handle with a communicator. */
int fe_step_policy(fe_handle* h, int n_steps, double beta, const fe_policy_rollout* rec /* or NULL */);
/* The drop-in env's step(u) (:91-109) as one launch and one wait, for small batches
 * where latency, not bandwidth, counts (FlockingRelativeEnv.step, N ~ 100-1000, B = 1).
 * u: (B,N,2) host actions, float32 or float64 (FE_U_F64). One env of at most one tile
 * (N <= 512) whose actions fit 3 KiB (N <= 384 in float32, 192 in float64) passes them in
 * the kernel arguments; otherwise page-locked ones (fe_host_alloc) are read by the kernel
 * in place, others copied first. Either way u may be reused on return. u == NULL: no dynamics,
 * compute_helpers (:111-134) on the current state (reset's observation). Outputs, any of
 * them NULL (not computed): state_values (B,N,6) f32, network (B,N,N) f32, rewards (B)
 * f64 and controls (B,N,2) f64 = controller() (:194-212) of the resulting state (fused,
 * FE_WITH_CONTROLLER implied). Page-locked destinations are written by the kernel
 * through their mapped addresses; others by a copy after it. Returns when all are in
 * place. Observations written to host arrays are not kept on the device (the device
 * getters then return GF_ESTATE); rewards also go to the ring (fe_get_rewards, metrics
 * path). flags: FE_U_F64, FE_WITH_CONTROLLER. */
int fe_step_host(fe_handle* h, const void* u, float* state_values, float* network, double* rewards,
                 double* controls, int flags);
/* Flocking-v0's drop-in step(u) (flocking.py:12-25 over flocking_relative.py:91-109) as
 * one call and one wait: fe_step_host (no controller) plus the new state's k nearest
 * neighbours (the selection fused into the step, or the kNN kernel), written to knn_idx
 * (B,N,K) int32 and knn_obs (B,N,4K) float32 (either may be NULL, not both): page-locked
 * destinations through their mapped addresses (both page-locked: the step and its rim
 * kNN write the rows there directly; otherwise one copy kernel or copies). Needs
 * n_neighbors > 0. Afterwards fe_get_knn returns the same rows (recomputed on the device
 * when they were written straight to the host). */
int fe_step_host_knn(fe_handle* h, const void* u, float* state_values, float* network, double* rewards,
                     int32_t* knn_idx, float* knn_obs, int flags);
/* Flocking-v0's drop-in expert loop, `u = env.controller(); env.step(u)` (controller()
 * inherited from flocking_relative.py:194-212 by flocking.py:5, step flocking.py:12-14):
 * fe_step_host_knn plus controls (B,N,2) f64 = controller() of the resulting state, fused
 * into the same launch (controls may be NULL: then as fe_step_host_knn). */
int fe_step_host_knn_ctrl(fe_handle* h, const void* u, float* state_values, float* network, double* rewards,
                          double* controls, int32_t* knn_idx, float* knn_obs, int flags);
/* controller(centralized) (:194-212) on the current state; centralized < 0 means the
 * config default. Writes (B,N,2) float64 to u_out (host) if non-NULL. */
int fe_controller(fe_handle* h, int centralized, double* u_out);
/* get_stats() (:136-143) on the current state: vel_diffs (N) and min_dists (N). */
int fe_get_stats(fe_handle* h, int env, double* vel_diffs, double* min_dists);
/* get_stats plus each agent's degree (r2 < comm_radius^2): reset()'s acceptance test
 * (:177-184) on the device. Any output pointer may be NULL. */
int fe_get_stats_ex(fe_handle* h, int env, double* vel_diffs, double* min_dists, int32_t* degree);
/* Per-env summaries of get_stats for the metrics path: dst (B,2) = np.mean(vel_diffs),
 * np.mean(min_dists) of every env's current state (flocking_relative.py:136-143), taken
 * on the device (a fixed summation tree: deterministic, ulps from NumPy's order). */
int fe_stats_summary(fe_handle* h, double* dst);

/* Outputs (host copies; env < 0 copies all B envs) ---------------------------- */
int fe_get_state_values(fe_handle* h, int env, float* dst);  /* (N,6) :128-129 */
int fe_get_network(fe_handle* h, int env, float* dst);       /* (N,N) :131-134 */
int fe_get_network_rows(fe_handle* h, int env, int row0, int nrows, float* dst);
/* Packed output of the last FE_PACKED_NETWORK step: bit j%64 of word j/64 of row i is
 * adj(i,j) (r2 < comm_radius^2, :117); the network is adj/max(degree,1) (:120-122).
 * env < 0: all envs. Either pointer may be NULL. */
int fe_get_network_packed(fe_handle* h, int env, uint64_t* bits, int32_t* degree);
int fe_get_controls(fe_handle* h, int env, double* dst);     /* (N,2) :210-211 */
int fe_get_rewards(fe_handle* h, double* dst);
/* The step's host outputs in one call with one stream sync (the drop-in env's
 * (state_values, network), reward tuple of step(), flocking_relative.py:109): any of
 * state_values (N,6) / network (N,N) of `env` (env < 0: all envs) and rewards (B) may be
 * NULL. flags: 0, or FE_OUT_MAPPED (page-locked destinations written by one copy
 * kernel: one launch instead of up to three DMA copies, each of which costs ~12-15 us of
 * latency at drop-in sizes). Returns after the data is in the destinations. */
int fe_get_outputs(fe_handle* h, int env, float* state_values, float* network, double* rewards, int flags);
/* Page-locked host memory for output arrays (the drop-in env hands such buffers to the
 * caller as fresh arrays and recycles them once released). */
int fe_host_alloc(size_t bytes, void** out);
int fe_host_free(void* p);               /* (B)   :145-147 */
int fe_get_knn(fe_handle* h, int env, int32_t* idx, float* obs); /* (N,k), (N,4k) */
int fe_device_buffers(fe_handle* h, fe_buffers* out);
/* How the plain step (no controller, variant, kNN or inline host actions; N % 4 == 0)
 * stores the dense network into the handle's buffer. The buffer holds the same dense
 * float32 network either way, bit for bit.
 *  FE_NET_DELTA (default): the library keeps a record of what the buffer holds (33 MiB at
 *    1024 x 256) and a step stores only the groups of the rows whose content changes.
 *    Every other kind of step stores in full, after which the next plain step stores in
 *    full once more to rebuild the record.
 *  FE_NET_FULL: every step stores every row in full and no record is kept.
 * The record costs a read and a write of N^2/8 bytes per env beside the 4 N^2 of the
 * network: where most groups change every step (a mean degree above N/4, where nearly
 * every 64-byte group holds a neighbour) the delta store moves up to 6.25 % more bytes
 * than the full one; choose FE_NET_FULL there. Measured on one MI355X at 1024 x 256
 * (profiles/delta_store/synthetic_full_vs_delta.json): a flock of mean degree 263 with
 * random actions runs 271.9 us per step with the delta store against 263.8 us in full
 * (3.1 % slower); nothing changing at all 142.9 against 170.2 us; the bench workload
 * 130.3 against 159.5 us ("Delta network store").
 * fe_buffers.network is read-only to callers: one that writes into it must call
 * fe_network_touched() before the next step, which then stores in full. */
#define FE_NET_DELTA 0
#define FE_NET_FULL 1
int fe_set_network_store(fe_handle* h, int mode);
int fe_network_touched(fe_handle* h);
int fe_sync(fe_handle* h);
/* Select a flocking variant for every later step / controller call (NULL: back to
 * FlockingRelative). */
int fe_set_variant(fe_handle* h, const fe_variant* v);
/* Per-env dt[B] for the following steps (FlockingStochastic-v0 draws one per step,
 * flocking_stoch.py:24); NULL reverts to cfg dt. */
int fe_set_dt(fe_handle* h, const double* dt);
/* FlockingStochastic-v0's dt ~ N(mean, sigma) of every step (flocking_stoch.py:20) drawn on
 * the device: NumPy's legacy np.random.normal on env b's own stream (fe_set_rng,
 * fe_reset_device), its cached second Gaussian included (fe_set_rng_gauss). NULL: off.
 * While the mode is on
 *  - fe_step (any action source or flags) first draws one dt per env, fe_step_expert
 *    n_steps per env (step t of env b integrates with the t-th), on the handle's stream
 *    after all of its outstanding work; the step then goes out as one launch behind the draw,
 *    as after fe_set_dt's upload. The variant code path is taken as with fe_set_dt.
 *  - GF_ESTATE from those calls if any env's stream was never seeded or set;
 *  - fe_step_host* return GF_ESTATE (the drop-in env draws on the host);
 *  - sigma == 0 still consumes the stream, as NumPy does.
 * GF_EINVAL for sigma < 0 or a non-finite value. fe_set_dt (NULL or an array) switches the
 * mode off; switching it on replaces a per-env dt set before. The uniforms, the rejection
 * test, the division and the square root are NumPy's bit for bit; the device's log may
 * differ from the host's in the last places, so a dt lies within sigma * |g| * 4 * 2^-52 +
 * 2^-53 * |dt| of NumPy's (g the standard Gaussian behind it). */
typedef struct fe_dt_noise { double mean, sigma; } fe_dt_noise;
int fe_set_dt_noise(fe_handle* h, const fe_dt_noise* noise /* NULL: off */);
/* The dts of the latest launch while the mode is on: (n_steps, B) after fe_step_expert,
 * (1, B) after fe_step. flags 0: dst is host memory, the call waits; FE_ROLLOUT_DEVICE: dst
 * is device memory, copied in stream order. GF_ESTATE before the first such launch (and
 * after the mode was switched off or on again). */
int fe_get_dt_steps(fe_handle* h, double* dst, int flags);

/* Multi-GPU metrics path (RCCL over xGMI) ---------------------- */
/* The env batch is sharded contiguously over ranks (one process per GPU); the
 * step path has no exchange. Only per-env rewards (and, optionally, get_stats
 * summaries) are all-gathered, on a side stream, so the collective never sits on the
 * step critical path. Shards may differ in size (shard.py's shard_range gives the first
 * B % world ranks one env more): every gathered block is padded to the largest shard,
 * max_envs, and rank r's entries past its own n_envs are zero. Every wait for a
 * collective is bounded by the init timeout: a rank that never joins or stops
 * responding makes the others' calls return GF_ECOMM (the communicator is then aborted
 * and the handle keeps stepping) instead of hanging. All ranks make the same sequence
 * of metrics calls after the same number of steps. */
int fe_comm_unique_id(uint8_t id[128]);
/* Creates the communicator (non-blocking RCCL init, polled) and all-gathers every
 * rank's n_envs (fe_comm_shard_sizes). Bounded by timeout_s (fe_comm_init: 300 s). */
int fe_comm_init(fe_handle* h, int nranks, int rank, const uint8_t id[128]);
int fe_comm_init_timeout(fe_handle* h, int nranks, int rank, const uint8_t id[128], double timeout_s);
/* The rule fe_comm_init applies to the exchanged sizes: GF_OK when every n_envs[r]
 * (r < nranks) is >= 1, else GF_ECOMM naming them. Host-only (no device). */
int fe_check_shard_sizes(int nranks, const int32_t* n_envs);
/* The communicator as RCCL sees it: ncclCommCount, ncclCommUserRank, the HIP device
 * ordinal it runs on (ncclCommCuDevice) and that device's PCI bus id (bus_id_len bytes,
 * hipDeviceGetPCIBusId). Any output pointer may be NULL. */
int fe_comm_info(fe_handle* h, int32_t* count, int32_t* user_rank, int32_t* device, char* bus_id, int bus_id_len);
/* Every rank's n_envs (sizes[nranks]) and the largest, the gathers' padded width. */
int fe_comm_shard_sizes(fe_handle* h, int32_t* sizes, int32_t* max_envs);
/* Enqueue (side stream, after the latest step) an all-gather of the per-env rewards of
 * every step since the previous reward all-gather (or since fe_comm_init), each step
 * exactly once, at any interval up to 64 steps. GF_ESTATE if no step was taken since,
 * or if more than 64 were (the oldest were overwritten: the call then skips them all). */
int fe_allgather_rewards(fe_handle* h);
/* Wait (bounded) for the latest reward all-gather; dst gets (nranks, steps, max_envs)
 * rewards, rank-major, steps = fe_gathered_steps(h) (oldest first). */
int fe_get_gathered_rewards(fe_handle* h, double* dst);
int fe_gathered_steps(fe_handle* h);
/* Enqueue (side stream) an all-gather of every rank's fe_stats_summary of the current
 * state: the optional get_stats aggregates of SURVEY.md §8e. The summaries are taken
 * on the handle's stream after both step halves (a join, so the next step is one launch,
 * unlike the reward all-gather); call it per episode or logging interval, not per step.
 * fe_get_gathered_stats waits (bounded) for it; dst gets (nranks, max_envs, 2),
 * rank-major. */
int fe_allgather_stats(fe_handle* h);
int fe_get_gathered_stats(fe_handle* h, double* dst);
/* Destroys the communicator and the metrics path's buffers; fe_comm_init may follow. A
 * side stream that does not drain within the collective timeout is aborted instead. */
int fe_comm_destroy(fe_handle* h);
/* Tests only: close = 1 enqueues on the collectives' side stream a one-wave kernel that
 * spins (s_sleep) until close = 0 is called or max_seconds pass, standing in for a
 * collective whose peer stopped responding; close = 0 releases it. Needs fe_comm_init. */
int fe_debug_comm_gate(fe_handle* h, int close, double max_seconds);
/* Tests only: what the metrics path saw, out[12]: [0] ring-slot reuse checks that found
 * a gather's staging copy still listed, [1] whether that copy had stored its completion
 * word at the last one (1) or not (0), [2] its bounded wait's status (-1: no wait), [3]
 * the communicator's async state at that wait's first poll, [4] staging copies listed
 * after the last reward gather, [5] whether its copy was complete right after the
 * gather was enqueued, [6] hipStreamQuery of the side stream right after the last gate
 * launch, [7] polls of the last bounded wait, [8] the gate kernel has started (1), [9]
 * how it ended (0 running, 1 opened, 2 timed out), [10] a communicator is live, [11]
 * staging copies listed now. */
int fe_debug_comm_state(fe_handle* h, int32_t* out);
/* The HIP runtime and RCCL this library is bound to in this process (a process that
 * loaded another copy of either first, e.g. PyTorch's bundled ones, binds that copy):
 * hipRuntimeGetVersion, hipDriverGetVersion (0 without a driver), ncclGetVersion, and the
 * paths of the shared objects those entry points resolved to (dladdr). Host-only; any
 * pointer may be NULL. */
int fe_runtime_info(int32_t* hip_runtime_version, int32_t* hip_driver_version, int32_t* rccl_version, char* hip_path,
                    int hip_path_len, char* rccl_path, int rccl_path_len);

/* ============================ Coverage-v0 ==================================== */
/* gym_flock/envs/spatial/coverage.py. B envs of n_robots robots moving on a per-env
 * target graph (at most max_nodes - n_robots targets). Node indices are global as in
 * the reference: robots 0..R-1, targets R..R+T-1. */
typedef struct cov_config {
  int32_t n_robots;        /* R (coverage.py:83, N_ROBOTS=6; config 4 uses 200)        */
  int32_t n_envs;          /* B                                                         */
  int32_t max_nodes;       /* padded node count (MAX_NODES :55; config 4 uses 1000)     */
  int32_t episode_length;  /* 75 (EPISODE_LENGTH :64)                                   */
  double res;              /* lattice spacing, edge-feature scale (DELTA 5.5, :80)       */
  double motion_radius;    /* res * 1.2 (:136)                                          */
  int32_t device;
  int32_t horizon;         /* greedy expert: relaxation sweeps - 1 (HORIZON=10, :66);
                              -1 = until converged                                       */
} cov_config;

typedef struct cov_handle cov_handle;

#define COV_ACTIONS_DEVICE   0x1 /* actions is a device pointer                          */
#define COV_ACTIONS_RESIDENT 0x2 /* use the actions last given to cov_set_actions        */
#define COV_ACTIONS_GREEDY   0x20 /* the step's actions are controller(greedy=True)'s (:800-872),
                                    computed in the same launch from per-node greedy lists
                                    built with the time matrix; robots the reference hands to
                                    np_random.choice(4) take action 0 (needs_random flags them),
                                    or with COV_GREEDY_RNG draw it on the device. The actions
                                    taken stay resident (COV_ACTIONS_RESIDENT). */
#define COV_GREEDY_RNG       0x80 /* with COV_ACTIONS_GREEDY: each fallback robot takes
                                    np_random.choice(4) (:861-864) from its env's stream (set
                                    by cov_set_rng), in robot order, bit-exact with numpy's
                                    legacy RandomState; the stream advances on the device */

int cov_create(const cov_config* cfg, cov_handle** out);        /* CoverageEnv.__init__ :83 */
int cov_destroy(cov_handle* h);
/* Targets of one env (env < 0: every env) and its motion graph + static observation
 * (_initialize_graph :529-594, utils._get_graph_edges :8-24), built on the device. */
int cov_set_targets(cov_handle* h, int env, int n_targets, const double* targets);

/* Per-episode target maps, _generate_targets (coverage.py:516-527) as every reset() calls
 * it (:378-397), with generate_lattice (make_map.py:30-67) and generate_geometric_roads
 * (make_map.py:207-231). The reference's values: arena (-120, 120, -120, 120) (XMAX/YMAX
 * :75-76), lattice_spacing DELTA = 5.5 (:61, the lattice vectors :125-128), 12 cities,
 * world_radius x_max, road_radius and link_radius motion_radius (= res * 1.2), near_radius
 * motion_radius / 1.4. */
typedef struct cov_map_config {
  double x_min, x_max, y_min, y_max; /* the arena: generate_lattice's free_region           */
  double lattice_spacing;            /* square lattice vectors (-s, 0), (0, -s)             */
  double world_radius;               /* cities U(-r, r)^2 (make_map.py:208)                 */
  double road_radius;                /* waypoint spacing along each Delaunay road (:228-229) */
  double near_radius;                /* lattice points within it of a waypoint (:521)       */
  double link_radius;                /* the target graph's radius (:523-524)                */
  int32_t n_cities;                  /* 12 (:518); at most 32                               */
} cov_map_config;
#define COV_MAP_SEED   0x1 /* seed env b's map stream as np.random.seed(map_seed + b) first;
                              otherwise the streams continue from the previous maps, as the
                              reference's global np.random does from one reset to the next */
#define COV_MAP_CITIES 0x2 /* the cities are given (host (n_sel, n_cities, 2), the drop-in
                              env draws them from np.random itself); no stream is used      */
/* status_out bits (per env) */
#define COV_MAP_NEAR_DEGENERATE 0x1 /* an orientation or incircle sign of the cities fell
                                       inside its rounding bound: Qhull decides such sets by
                                       its own precision handling (parity unpinned)         */
#define COV_MAP_TOO_MANY        0x2 /* more targets than max_nodes - n_robots              */
#define COV_MAP_TOO_FEW         0x4 /* fewer targets than robots                           */
#define COV_MAP_OVERFLOW        0x8 /* more waypoints than the kernel holds: its capacity is
                                       the bound for cities in general position inside
                                       world_radius (n_cities + (3 n_cities - 6) roads of at
                                       most the square's diagonal), less if the LDS is
                                       short. Cocircular cities (up to n (n - 1) / 2 roads,
                                       all of them kept), given cities outside
                                       world_radius or a tiny road_radius can exceed it;
                                       a road whose waypoint count is above it, not a
                                       number or beyond an int is reported the same way */
/* New maps on the device for env `env` (env < 0: every env): the cities (drawn on the
 * device from each env's stream, numpy's legacy uniform, or given), their Delaunay roads,
 * the lattice points near them and the largest connected component of their radius
 * graph; then the motion graph and static observation as cov_set_targets builds them.
 * n_targets_out, status_out (n_sel) and cities_out (n_sel, n_cities, 2) may be NULL. A
 * map that cannot be used (TOO_MANY / TOO_FEW / OVERFLOW) fails the call with GF_EINVAL,
 * that env left without a graph; NEAR_DEGENERATE maps are used and reported. A map is
 * never built from a shortened road list: every pair of up to 32 cities can be a road (the
 * cocircular case), and a map whose waypoints do not fit is OVERFLOW. Given cities must be
 * finite: a NaN or an infinity fails the call with GF_EINVAL before anything is launched. */
int cov_generate_maps(cov_handle* h, const cov_map_config* mc, int env, uint64_t map_seed, const double* cities,
                      int flags, int32_t* n_targets_out, int32_t* status_out, double* cities_out);
/* The targets (n_targets, 2) of env `env`'s current map. */
int cov_get_targets(cov_handle* h, int env, double* targets);
/* Host only (no device): generate_lattice's points (make_map.py:30-67) for mc, [y, x]
 * columns in its order, into xy (capacity *n points; *n receives the count, also when
 * the capacity is short, which fails with GF_EINVAL). xy may be NULL to query *n. */
int cov_map_lattice(const cov_map_config* mc, double* xy, int32_t* n);

/* ----- CoverageARL-v0 / CoverageFull-v0 (gym_flock/envs/spatial/coverage_arl.py) -----
 * The targets come from an occupancy grid (make_map.from_occupancy, make_map.py:234-271):
 * free cells within perimeter_delta cells of an occupied one, as points ((cell * res) +
 * xyz_min) + res / 2 with res = 0.5 * downsample_rate, rotated (x, y) = (t_y, -t_x), and
 * with check_connected the largest component of their radius graph (load_graph,
 * coverage_arl.py:46-62; the handle's motion_radius). That pool is shared by every env of
 * the handle. With num_subgraphs > 1 every reset() samples a random window of
 * (max_xy - min_xy) / num_subgraphs of it and keeps the window's largest component,
 * until one holds min_targets points (_generate_targets, coverage_arl.py:64-83). */
typedef struct cov_occupancy_config {
  int32_t downsample_rate;   /* 10 (the reference's grid_slice10 map)                     */
  double perimeter_delta;    /* 2.0, in cells                                             */
  double xyz_min[2];         /* (-321.0539855957031, -276.5395050048828) (make_map.py:264) */
  int32_t check_connected;   /* keep the pool's largest component (coverage_arl.py:49-54)  */
  double num_subgraphs;      /* 3.0; <= 1: no sampling, the map is the whole pool          */
  int32_t min_targets;       /* MIN_GRAPH_SIZE = 200 (coverage_arl.py:10)                  */
  int32_t max_tries;         /* bound of the sampler's retry loop on the streams (4096);
                                the reference's loop is unbounded                          */
} cov_occupancy_config;
#define COV_MAP_DRAWS     0x4  /* cov_generate_submaps: the graph_start draws are given     */
#define COV_MAP_NO_WINDOW 0x10 /* status bit: no try gave a component of min_targets points */
#define COV_POOL_CAP      8192 /* pool points before the component step; also the most
                                  targets per map (max_nodes - n_robots) every Coverage
                                  path holds: pool, motion graph, seeded reset, time matrix,
                                  greedy controller, hidden-node observation. The fused
                                  expert forms (COV_ACTIONS_GREEDY, cov_step_expert,
                                  COV_NEXT_GREEDY) keep their own limit of 1024. */
/* The target pool of grid (n0, n1) bytes, nonzero = occupied, on the device (one launch).
 * *n_pool_out (may be NULL) receives the pool's size. GF_EINVAL, before any launch, for a
 * grid without an occupied cell or one that may give more than COV_POOL_CAP points. */
int cov_load_occupancy(cov_handle* h, const cov_occupancy_config* cfg, const uint8_t* grid, int n0, int n1,
                       int32_t* n_pool_out);
/* The pool (n_pool, 2) in cell order (all_targets), min_xy[2], max_xy[2] and
 * subgraph_size[2] = (max_xy - min_xy) / num_subgraphs; any may be NULL. Host copies. */
int cov_get_pool(cov_handle* h, double* targets, double* min_xy, double* max_xy, double* subgraph_size);
/* A new sampled map for env `env` (env < 0: every env), then its motion graph and static
 * observation as cov_set_targets builds them. The draws graph_start = low + (high - low) *
 * u (low = min_xy, high = max_xy - subgraph_size; x, then y: two doubles per try) come
 * from each env's map stream (the streams of cov_generate_maps; COV_MAP_SEED seeds env
 * b's as np.random.seed(map_seed + b) first), at most max_tries tries; or with
 * COV_MAP_DRAWS from draws (n_sel, n_draws, 2), the graph_start values themselves (what
 * np.random.uniform(low, high, size=(n_draws, 1, 2)) returns), at most n_draws tries.
 * n_targets_out, status_out, tries_out (n_sel; may be NULL): the accepted component's size,
 * the status bits, the tries consumed. On the streams an env left without a window
 * (COV_MAP_NO_WINDOW) fails the call with GF_EINVAL like TOO_MANY / TOO_FEW (judged on the
 * accepted component), that env left without a graph; with COV_MAP_DRAWS a list that gave
 * no window is reported in status_out only (the caller draws again). GF_ESTATE without a
 * pool, GF_EINVAL with num_subgraphs <= 1 (the map is the pool: cov_set_targets). */
int cov_generate_submaps(cov_handle* h, int env, uint64_t map_seed, const double* draws, int n_draws, int flags,
                         int32_t* n_targets_out, int32_t* status_out, int32_t* tries_out);

/* reset() after its random draws (:405-424): start[B][R] target-local start nodes,
 * visited[B][max_nodes-R] (1 = visited); computes reset's observation (:424). */
int cov_reset(cov_handle* h, const int32_t* start, const uint8_t* visited);
/* reset() with its random draws on the device (:405-424): env b as a reference env whose
 * np_random was seeded seed + b, RandomState(seed + b)'s choice(arange(T), R,
 * replace=False) for the start targets and choice(arange(T) + R, int(T * frac_active),
 * replace=False) for the unvisited ones, bit-exact; the envs' streams then continue on the
 * device for COV_GREEDY_RNG (as after cov_set_rng). start_out (B,R) and visited_out
 * (B, max_nodes - R) may be NULL; otherwise they receive the draws, in cov_reset's layout.
 * GF_EINVAL where the draws' LDS (2496 + 9 * (max_nodes - R) bytes) exceeds a CU's 160 KB
 * (above 17,927 targets: draw on the host, cov_reset). */
int cov_reset_seeded(cov_handle* h, uint64_t seed, double frac_active, int32_t* start_out, uint8_t* visited_out);

/* reset() of chosen envs on the device, their np_random streams continued, with the
 * reference's nearby_starts region (coverage.py:398-414, :596-599, get_n_nearest :655-673). */
#define COV_RESET_SEED      0x1  /* selected env b starts from RandomState(seed + b); else its stream continues */
#define COV_RESET_NEW_MAPS  0x2  /* selected envs first draw a new map from their own map streams */
#define COV_RESET_DONE      0x4  /* env_mask == NULL selects the envs whose done flag is set */
/* status bits per selected env */
#define COV_RESET_REGION_SHORT 0x1  /* the region stopped growing below `nearby` nodes (the reference would loop forever) */
#define COV_RESET_REGION_SMALL 0x2  /* fewer region nodes than robots (numpy raises): env not reset, call fails */

typedef struct {
  double   frac_active;  /* frac_active_targets, [0,1] */
  int32_t  nearby;       /* 0: every target may be a start; n > 0: get_n_nearest(choice(T), n) */
  int32_t  flags;
  uint64_t seed;         /* COV_RESET_SEED */
} cov_reset_config;

/* The envs with env_mask[b] != 0 (env_mask NULL: every env, or with COV_RESET_DONE the envs
 * whose done flag is set) are reset; every other env stays as it is, bit for bit: its
 * observation (the hidden one included), robots, visited flags, step counter, reward / done,
 * resident actions, np_random and map streams, map and time matrix. A selected env b draws
 * from its np_random stream on the device (cov_set_rng / cov_reset_seeded, or seeded here:
 * COV_RESET_SEED), in the reference's order:
 *   1. nearby > 0: i = np_random.choice(T), one scalar draw (none when T == 1);
 *   2. region = {i}; while |region| < nearby: region |= out-neighbours(region) in the motion
 *      graph, each round from the set as it stood at its start (the set may overshoot
 *      nearby). A round that adds nothing ends the loop: COV_RESET_REGION_SHORT;
 *   3. start = members_ascending[permutation(|region|)[:R]]; with nearby == 0 the members are
 *      all T targets and the draws are cov_reset_seeded's;
 *   4. unvisited = permutation(T)[:int(T * frac_active)];
 *   5. cov_reset's pass and observation for the env (discovered := robots on a hidden handle).
 * COV_RESET_NEW_MAPS: the selected envs first draw their next map from their own map streams,
 * with cov_generate_submaps' sampler when a pool with num_subgraphs > 1 is loaded, else with
 * the configuration of the last cov_generate_maps call that drew its cities (GF_ESTATE
 * without either); only their time matrices and greedy lists become invalid.
 * Outputs (any may be NULL; rows of unselected envs are left untouched): start_out (B,R),
 * visited_out and region_out (B, max_nodes - R; region: 1 = a node of the start region),
 * status_out (B), *n_reset_out the envs reset. An env with fewer region nodes than robots
 * (COV_RESET_REGION_SMALL) keeps its previous state, though its stream has advanced by the
 * scalar draw (its start_out row reads -1, its visited_out row 1); the other selected envs
 * are reset and the call returns GF_EINVAL naming it.
 * GF_ESTATE: no streams on the device without COV_RESET_SEED; COV_RESET_DONE before any
 * reset; a first reset that does not take every env. With COV_RESET_DONE and nothing done:
 * no launch, *n_reset_out = 0, GF_OK. GF_EINVAL before any device work: frac_active outside
 * [0,1], nearby < 0, unknown flags, seed + n_envs above 2^32, n_robots > 624, or the draws'
 * LDS (2496 + 9 * (max_nodes - R) + 16 * ceil((max_nodes - R) / 64) bytes) above a CU's
 * 160 KB (above 17,441 targets). */
int cov_reset_device(cov_handle* h, const cov_reset_config* rc, const uint8_t* env_mask /* (B) or NULL */,
                     int32_t* start_out /* (B,R) */, uint8_t* visited_out /* (B,max_nodes-R) */,
                     uint8_t* region_out /* (B,max_nodes-R) */, int32_t* status_out /* (B) */,
                     int32_t* n_reset_out);
/* step(action) (:174-204, :234-364): actions[B][R] in [0,4). */
int cov_step(cov_handle* h, const int32_t* actions, int flags);
/* n_steps fused greedy expert steps (COV_ACTIONS_GREEDY | COV_GREEDY_RNG: controller(greedy=
 * True)'s actions and the reference's np_random.choice(4) fallback draws, coverage.py:800-872,
 * then step, :174-364) in ONE launch, each env's workgroup stepping its env n_steps times:
 * the same result as n_steps calls of cov_step(h, NULL, COV_ACTIONS_GREEDY | COV_GREEDY_RNG)
 * (expert rollouts: the reference's demonstrations). Needs the envs' streams on the device
 * (cov_set_rng / cov_reset_seeded), n_robots <= 624 and max_nodes - n_robots <= 1024.
 * rewards / done (both may be NULL; then the call returns without waiting): (n_steps, B) host
 * arrays of every step's reward and done flag; the last step's are also cov_get_rewards'. */
int cov_step_expert(cov_handle* h, int n_steps, double* rewards, uint8_t* done);
int cov_set_actions(cov_handle* h, const int32_t* actions);
/* Every env's np_random stream for COV_GREEDY_RNG steps, in the layout of numpy's
 * RandomState.get_state() (MT19937): keys[B][624] the key words, pos[B] in [0, 624] the
 * position. Needs n_robots <= 624. cov_get_rng reads them back (after the steps that
 * drew from them), to continue the stream on the host with RandomState.set_state. */
int cov_set_rng(cov_handle* h, const uint32_t* keys, const int32_t* pos);
int cov_get_rng(cov_handle* h, uint32_t* keys, int32_t* pos);
/* The drop-in env's step(action) (coverage.py:174-204 with _get_obs_reward :234-364) as
 * one launch and one wait, the reference driver's loop (test.py:43-74): actions[B][R] in
 * [0,4) (B*R <= 512: passed in the kernel arguments), then the whole observation of every
 * env, step counter, reward, done flag and each robot's node after the step (the next
 * step's last_loc, closest_targets :427-432) written to the given host arrays: nodes
 * (B,M,3) f32, edges (B,4M) f32, senders / receivers (B,4M) i32, step (B) i64, reward (B)
 * f64, done (B) u8, closest (B,R) i32. Page-locked destinations (fe_host_alloc) are
 * written by the step's own workgroups through their mapped addresses, others by copies
 * after it; any pointer may be NULL. flags: COV_NEXT_GREEDY also computes, in the same
 * launch, controller(greedy=True)'s actions of the resulting state (:800-872) into
 * next_actions (B,R) i32 and needs_random (B,R) u8 (robots the reference hands to
 * np_random.choice(4), action 0 here), which also stay resident (COV_ACTIONS_RESIDENT);
 * it builds the time matrices first if the graph changed. */
#define COV_NEXT_GREEDY 0x40
int cov_step_host(cov_handle* h, const int32_t* actions, float* nodes, float* edges, int32_t* senders,
                  int32_t* receivers, int64_t* step, double* reward, uint8_t* done, int32_t* closest,
                  int32_t* next_actions, uint8_t* needs_random, int flags);
/* Place one env's robots anywhere (x[:R] = ...); closest targets are recomputed. */
int cov_set_robot_positions(cov_handle* h, int env, const double* xr);
/* Observation of one env (:353): nodes (M,3) f32, edges (4M) f32, senders/receivers
 * (4M) i32, step; any pointer may be NULL. */
int cov_get_obs(cov_handle* h, int env, float* nodes, float* edges, int32_t* senders, int32_t* receivers,
                int64_t* step);
int cov_get_rewards(cov_handle* h, double* reward, uint8_t* done);   /* (B), (B) */
int cov_get_robots(cov_handle* h, int env, double* xr, int32_t* nodes); /* closest_targets :427 */
int cov_get_visited(cov_handle* h, int env, uint8_t* visited); /* (max_nodes - R): reset()'s layout */
int cov_get_n_motion(cov_handle* h, int32_t* n_motion);
int cov_get_n_targets(cov_handle* h, int32_t* n_targets); /* (B) targets of each env's current map (0: none) */
/* Launches per cov_step. n = 0 (the default): fused greedy steps (COV_ACTIONS_GREEDY) go
 * out as two half-batch launches on two streams (as fe_set_streams), every other step as
 * one launch, which the device, not the host, bounds (scripts/cov_launch_probe.py); n = 2
 * splits every step, n = 1 none. Every other call, cov_sync included, first orders the
 * handle's stream after both. */
int cov_sync(cov_handle* h);
int cov_set_streams(cov_handle* h, int n);
/* How the time matrix is built (diagnostics and tests; the default chooses by size). One
 * wave keeps the rows of sources_per_wave sources in LDS, (n_targets + 1) * sources_per_wave
 * entries of one byte, or of two where a hop count passes 254: 0 takes the largest of 64,
 * 32, 16, 8 that fits a CU's 160 KB for the largest map of a build (64 up to 2,559 targets,
 * 16 and 8 at 8,192), another value caps it (GF_EINVAL unless 8, 16, 32 or 64, or if one
 * byte per entry of max_nodes - n_robots + 1 targets does not fit; the two-byte rerun
 * narrows the tile by itself where it must). schedule_in_global = 1 keeps the edge
 * schedule's working arrays in device memory, as maps whose (2 n_targets + 4 n_edges + 4)
 * words exceed the LDS do anyway. Every choice gives the same matrices. Takes effect at the
 * next build and marks every env's matrix stale. */
int cov_set_tm_plan(cov_handle* h, int sources_per_wave, int schedule_in_global);
/* Greedy expert, controller(greedy=True) :800-872. On first use after cov_set_targets
 * it builds each env's time matrix (construct_time_matrix :621-653) on the device;
 * then every robot heads for its nearest unvisited target via the predecessor matrix.
 * The actions stay resident for cov_step(.., COV_ACTIONS_RESIDENT). Robots the
 * reference hands to np_random.choice(4) (target out of reach, :839-844 and :863-864)
 * get action 0 and needs_random = 1: draw those on the host in robot order and upload
 * the patched array with cov_set_actions. actions[B][R], needs_random[B][R] and
 * n_random may be NULL; with all three NULL the call does not synchronise. Maps of up to
 * COV_POOL_CAP targets; GF_EINVAL above. */
int cov_controller_greedy(cov_handle* h, int32_t* actions, uint8_t* needs_random, int64_t* n_random);
/* The resident actions (B,R) (the last cov_set_actions, cov_controller_greedy or
 * COV_ACTIONS_GREEDY step) and the needs_random flags (B,R) of the last greedy call;
 * either pointer may be NULL. */
int cov_get_actions(cov_handle* h, int32_t* actions, uint8_t* needs_random);
/* One env's graph_cost (inf -> MAX_COST=1000, as :651) and graph_previous, each
 * (T,T) row-major, T = that env's target count; builds the matrix if needed. */
int cov_get_time_matrix(cov_handle* h, int env, int32_t* cost, int32_t* prev);

/* Observation wire formats for graph trainers. */
#define COV_OUT_DEVICE 0x4 /* output pointers are device memory (else host)             */
#define COV_FLAT_F32   0x8 /* flat rows as float32 (the wrapper's Box dtype), else float64 */
#define COV_MASK_ALL   0x10 /* graph tuple: drop every graph's padded edges, not only graph
                               0's as the reference's unpack_obs does (see below)         */
/* Every env's observation flattened like gym's FlattenDictWrapper over keys
 * ['nodes','edges','senders','receivers','step'] (coverage.py:90, test.py:33):
 * dst (B, 15*max_nodes + 1), float64 (np.concatenate's promotion) or float32. */
int cov_get_flat_obs(cov_handle* h, void* dst, int flags);
/* unpack_obs (coverage.py:689-741) of the batch without TensorFlow: n_edge[B] and the
 * total edge count of the tuple cov_get_graphs_tuple writes. The reference masks edges
 * after offsetting senders by the graph's first node, so only graph 0 drops its padding
 * (COV_MASK_ALL drops all). */
int cov_graphs_tuple_sizes(cov_handle* h, int32_t* n_edge, int64_t* total_edges, int flags);
/* n_node[B] (= max_nodes), nodes (B*max_nodes, 3) f32, n_edge[B], edges (total, 1) f32,
 * senders/receivers (total) i32 offset by b*max_nodes, globs (B, 1) f32 (step). Any
 * pointer may be NULL; with COV_OUT_DEVICE all are device pointers. */
int cov_get_graphs_tuple(cov_handle* h, int32_t* n_node, float* nodes, int32_t* n_edge, float* edges,
                         int32_t* senders, int32_t* receivers, float* globs, int flags);

/* Hidden nodes (ExploreEnv-v0 / -v1: hide_nodes=True, n_node_feat=4; coverage.py:334-346).
 * enable = 1 allocates the hidden observation and sets every env's discovered set to the
 * robots only; from then on every call that makes an observation (cov_reset,
 * cov_reset_seeded, cov_step with host, device or resident actions) is followed on the
 * handle's stream by a pass that
 *   - adds to the env's discovered set every target within 0 < r <= 4 * 5.5 of a robot (the
 *     reference's module constant DELTA, whatever the env's res; a robot does not see the
 *     node it stands on, r = 0),
 *   - writes the node rows (max_nodes, 4): the three features times the discovered flag,
 *     then the frontier flag (1 on a discovered receiver of an edge slot whose sender is
 *     undiscovered, over all 4 * max_nodes slots),
 *   - writes the senders with -1 in every slot that has an undiscovered end, the last
 *     8 * n_robots action-edge slots excepted.
 * cov_reset / cov_reset_seeded set discovered back to the robots only before their
 * observation, and so do cov_set_targets, cov_generate_maps and cov_generate_submaps for
 * the envs they touch; cov_set_robot_positions leaves it alone. On such a handle
 *   - cov_get_obs keeps returning the unhidden 3-feature observation,
 *   - cov_controller_greedy masks visited OR undiscovered targets (controller :817-821,
 *     with its np.where quirk: target 0 is masked too once any target is masked),
 *   - cov_get_flat_obs rows are 16 * max_nodes + 1 wide (nodes (max_nodes, 4), edges, the
 *     hidden senders, receivers, step), and the graph tuple has (B * max_nodes, 4) nodes
 *     and drops the slots whose hidden sender is -1 (graph 0 only, or all: COV_MASK_ALL),
 *   - the fused expert forms (COV_ACTIONS_GREEDY, COV_NEXT_GREEDY, cov_step_expert,
 *     cov_step_host) return GF_EINVAL: they read the visited flags inside the step.
 *     cov_explore_expert (below) is the fused expert form for such a handle.
 * enable = 0 turns the pass off again. A handle that never enables it launches and
 * allocates nothing for it. */
int cov_set_hidden(cov_handle* h, int enable);
/* The hidden observation of one env: nodes4 (max_nodes, 4) f32, senders (4 * max_nodes)
 * i32, discovered (max_nodes) u8. Any pointer may be NULL. Edges, receivers and step are
 * cov_get_obs'. GF_ESTATE when the handle does not hide nodes. */
int cov_get_hidden_obs(cov_handle* h, int env, float* nodes4, int32_t* senders, uint8_t* discovered);
/* Expert rollouts of a handle that hides nodes (ExploreEnv), recorded: n_steps of
 *   controller(greedy=True) with hide_nodes (the expert masks visited OR undiscovered targets,
 *   its np_random.choice(4) fallback draws from the env's device stream, coverage.py:800-872),
 *   step (:174-364), and the discovery from the robots' new positions (:334-346)
 * in ONE launch, each env's workgroup stepping its env n_steps times with the discovered set
 * in LDS. Afterwards the handle is exactly as after n_steps times (cov_controller_greedy,
 * the fallback robots' draws in robot order, cov_set_actions, cov_step(COV_ACTIONS_RESIDENT)):
 * every getter, the streams (cov_get_rng) and every later call see the same bits. The full
 * hidden observation (node rows, frontier flags, hidden senders) is only rewritten after the
 * last step and after the steps whose flat row is recorded.
 * Records (any pointer may be NULL; rec may be NULL): */
typedef struct cov_rollout {
  double*  rewards;       /* (n_steps,B)   every step's                                   */
  uint8_t* done;          /* (n_steps,B)                                                  */
  int32_t* actions;       /* (n_steps,B,R) the expert's actions, fallback draws included  */
  uint8_t* needs_random;  /* (n_steps,B,R) 1 where the action was drawn                   */
  float*   flat_obs;      /* (K,B,16*max_nodes+1) hidden FlattenDictWrapper row after step t,
                             for every t with (t+1) % record_every == 0. On a handle that
                             does not hide nodes (cov_expert_rollout) the row is
                             15*max_nodes+1 wide.                                         */
  int32_t  record_every;  /* >= 1 and divides n_steps; K = n_steps / record_every         */
  int32_t  flags;         /* COV_ROLLOUT_DEVICE: pointers are caller-owned device memory  */
} cov_rollout;
#define COV_ROLLOUT_DEVICE 0x1
/* Pairing for imitation learning: the row recorded after step t is the observation the expert
 * saw when it chose actions[t + 1]; the observation for actions[0] is cov_get_flat_obs (with
 * COV_FLAT_F32) before the call. With rec == NULL or COV_ROLLOUT_DEVICE the call only
 * enqueues (device destinations are written by the kernel in stream order; cov_sync before
 * reading them); host destinations go through the handle's scratch and the call returns when
 * they are in place. Before any device work: GF_ESTATE when the handle does not hide nodes,
 * has not been reset or has no device streams (cov_set_rng / cov_reset_seeded); GF_EINVAL
 * for n_steps < 1, record_every < 1 or not a divisor of n_steps, unknown flags, n_robots >
 * 624, more LDS than 64 KB per workgroup (cov_explore_lds_bytes), or max_nodes - n_robots >
 * 1024 (the greedy lists, as for the other fused forms). */
int cov_explore_expert(cov_handle* h, int n_steps, const cov_rollout* rec /* or NULL */);
/* The LDS bytes a workgroup of cov_explore_expert takes for n_robots and max_nodes: the step's
 * region, the hidden pass's and 16 bytes per target (host arithmetic only, no device). */
int64_t cov_explore_lds_bytes(int n_robots, int max_nodes);

/* n_steps greedy expert steps of a handle that does NOT hide nodes in one launch, recorded,
 * across episode ends: the reference driver's loop `reset(); while not done: a =
 * controller(greedy=True); step(a)` for every env of the batch, its output the demonstrations
 * for imitation learning. Records: cov_rollout (above), rows 15 * max_nodes + 1 wide.
 *
 * Without ar the handle afterwards is exactly as after n_steps calls of cov_step(h, NULL,
 * COV_ACTIONS_GREEDY | COV_GREEDY_RNG): rewards and done equal cov_step_expert's, and every
 * getter, cov_get_rng and every later call see the same bits; an env steps on past done.
 *
 * With ar an env is reset inside the launch right after a step of this call sets its done
 * flag, on its unchanged map (coverage.py:398-424 with graph_changed == False), drawing from
 * its own np_random stream where the step left it: the handle afterwards is exactly as after
 * n_steps rounds of that step, each followed by cov_reset_device(h, {frac_active, nearby,
 * COV_RESET_DONE, 0}, NULL, ...) whose GF_EINVAL for a too-small region is ignored. An env
 * that is already done on entry is simply stepped. An env whose start region has fewer nodes
 * than robots (COV_RESET_REGION_SMALL) keeps its state, has its stream advanced by the scalar
 * draw, gets the bit in status[b] and goes on stepping; it is not counted in n_resets[b], and
 * the call still returns GF_OK (a call that only enqueues cannot fail late). */
typedef struct {
  double   frac_active;  /* as cov_reset_config */
  int32_t  nearby;       /* as cov_reset_config */
  int32_t  flags;        /* must be 0: no seeding, no new maps inside a launch */
  int32_t* n_resets;     /* (B) resets of env b made by this call, or NULL */
  int32_t* status;       /* (B) OR of the COV_RESET_REGION_* bits of those resets, or NULL */
} cov_auto_reset;
/* Pairing for imitation learning: the row recorded after step t is the observation the expert
 * saw when it chose actions[t + 1]; after a step that set done it is the reset observation, so
 * done[t] marks the last step of an episode, rewards[t] is that step's reward, and the
 * terminal observation is not recorded. The observation for actions[0] is cov_get_flat_obs
 * (with COV_FLAT_F32) before the call. COV_ROLLOUT_DEVICE in rec->flags also governs
 * ar->n_resets and ar->status. With rec == NULL (and no host destination in ar) or
 * COV_ROLLOUT_DEVICE the call only enqueues; host destinations go through the handle's
 * scratch and the call returns when they are in place. Before any device work: GF_ESTATE
 * when the handle has not been reset or has no device streams (cov_set_rng /
 * cov_reset_seeded); GF_EINVAL for a handle that hides nodes (cov_explore_expert is its
 * form), n_steps < 1, record_every < 1 or not a divisor of n_steps, unknown rec->flags,
 * ar->flags != 0, frac_active outside [0,1], nearby < 0, n_robots > 624, max_nodes -
 * n_robots > 1024 (the greedy lists), or more LDS than 64 KB per workgroup
 * (cov_rollout_lds_bytes). */
int cov_expert_rollout(cov_handle* h, int n_steps, const cov_rollout* rec /* or NULL */,
                       const cov_auto_reset* ar /* NULL: no reset, envs step on past done */);
/* The LDS bytes a workgroup of cov_expert_rollout takes: the step's region and, with
 * auto_reset, the reset draws' (key, permutation, draws, two bit sets, flags). Host
 * arithmetic only, no device. */
int64_t cov_rollout_lds_bytes(int n_robots, int max_nodes, int auto_reset);

/* Graph helpers of gym_flock/envs/spatial/utils.py ------
 * A context owns device scratch and the last edge list. Positions are host float64
 * (n, 2) arrays; pos2 == NULL means pos2 = pos1 (the reference's pos2=None), with the
 * diagonal as the self pair. Edges come out in np.nonzero's row-major order. */
typedef struct gu_graph gu_graph;
int gu_create(int device, gu_graph** out);
int gu_destroy(gu_graph* g);
/* _get_graph_edges(rad, pos1, pos2=None, self_loops=False), utils.py:8-24: pairs with
 * r = |pos1[i] - pos2[j]| != 0 and not r > rad. *n_edges = their count. */
int gu_radius_edges(gu_graph* g, const double* pos1, int32_t n1, const double* pos2, int32_t n2, double rad,
                    int self_loops, int64_t* n_edges);
/* _get_k_edges(k, pos1, pos2=None, self_loops=False, allow_nearest=False),
 * utils.py:60-88: per row the k smallest r (allow_nearest), or the k+1 smallest minus
 * the row's argmin. Equal distances at the k-th boundary go to the lower column (numpy
 * leaves that choice to its selection algorithm). GF_EINVAL where np.argpartition
 * raises (kth >= row length). */
int gu_k_edges(gu_graph* g, int32_t k, const double* pos1, int32_t n1, const double* pos2, int32_t n2,
               int self_loops, int allow_nearest, int64_t* n_edges);
/* The last result: senders/receivers (E) i32, r (E) f64, diff (2E) f64 = every edge's
 * dx, then every dy (the reference's np.hstack of the two difference columns). Any
 * pointer may be NULL. */
int gu_get_edges(gu_graph* g, int32_t* senders, int32_t* receivers, double* r, double* diff);
/* _nodes_within_radius(rad, pos1, pos2), utils.py:27-39: valid[j] = 1 when the column
 * sum of r (r > rad zeroed) over pos1 is > 0. */
int gu_nodes_within_radius(gu_graph* g, const double* pos1, int32_t n1, const double* pos2, int32_t n2, double rad,
                           uint8_t* valid);

/* Shepherding-v0 (gym_flock/envs/shepherding/shepherding.py) ----------------------
 * B envs of N = n_shepherds + n_sheep unicycle agents, state (B,N,3) float64 =
 * [x, y, theta], shepherds first. One launch per call: the step (:80-117) with the sheep's
 * repulsion controller (:164-178, summed over j in order like np.sum), then the new
 * state's observation (B,N,4) = [x, y, theta, identity] (:127), adjacency (B,N,N) =
 * 1/r within comm_radius, 0 on the diagonal and beyond (:139-162), and reward (B) = the
 * fraction of sheep with |(x, y)| < goal_region_radius (:180-185), all float64. The
 * adjacency, the reward and the sheep's controls are bit-exact for a given state; cos, sin
 * and atan2 are the device library's, so the integrated state and the shepherd controller
 * match NumPy to rounding. One stream per handle; every call is ordered on it. */
typedef struct shep_config {
  int32_t n_shepherds;          /* 10 (:28)                                          */
  int32_t n_sheep;              /* 20 (:27); n_shepherds + n_sheep <= 1024           */
  int32_t n_envs;               /* B                                                 */
  double dt;                    /* 0.01 (:33)                                        */
  double comm_radius;           /* 2.0 (:46)                                         */
  double action_scalar;         /* 5.0 (:35)                                         */
  double force_weight_shepherd; /* 0.15 * 3.0 (:50), as the host computed it         */
  double force_weight_sheep;    /* 0.15 * 0.5 (:50)                                  */
  double goal_region_radius;    /* 0.5 * (1.0 * sqrt(N)) (:39, :43)                  */
  int32_t device;               /* HIP device ordinal                                */
} shep_config;
typedef struct shep_handle shep_handle;

#define SHEP_U_DEVICE   0x02 /* u is a device pointer (else host)                          */
#define SHEP_U_F64      0x04 /* u is float64 (else float32): u * action_scalar (:89) is
                                computed in u's precision, as NumPy does                   */
#define SHEP_U_EXPERT   0x08 /* u := controller() of the current state, in the same launch */
#define SHEP_U_RESIDENT 0x80 /* u := the handle's action buffer: the last host actions or
                                the last shep_controller output                            */
#define SHEP_OUT_DEVICE 0x4  /* dst is device memory (else host); stream-ordered, shep_sync */
#define SHEP_OUT_F32    0x8  /* dst is float32 (else float64)                               */

/* GF_EINVAL before any device work for a null pointer, n_shepherds < 1, n_sheep < 1,
 * N > 1024, n_envs < 1 and a non-positive dt, comm_radius or goal_region_radius. */
int shep_create(const shep_config* cfg, shep_handle** out);
int shep_destroy(shep_handle* h);
int shep_set_state(shep_handle* h, const double* x);   /* (B,N,3) host */
int shep_get_state(shep_handle* h, double* x);
/* Observation, adjacency and reward of the state just set (reset() :187-202). */
int shep_observe(shep_handle* h);
/* One step. u: (B,n_shepherds,2) shepherd actions in host memory (copied to the handle's
 * action buffer), or device memory (SHEP_U_DEVICE, read in place on the handle's stream),
 * or NULL with SHEP_U_RESIDENT / SHEP_U_EXPERT. GF_ESTATE before a state is set. */
int shep_step(shep_handle* h, const void* u, int flags);
/* controller() :204-273 of the current state into the handle's action buffer (float64);
 * out (B,n_shepherds,2) host or NULL (then no synchronisation). The quirk of :253 is kept:
 * a shepherd is tested for line of sight only when exactly one of the two states has a
 * component that is exactly zero. */
int shep_controller(shep_handle* h, double* out);
/* n_steps of u = controller(); step(u) in one launch, the state held in LDS throughout;
 * every step's reward to rewards (n_steps,B) host or NULL (then no synchronisation); the
 * observation and adjacency are the last step's. */
int shep_step_expert(shep_handle* h, int n_steps, double* rewards);
/* The last observation (B,N,4), adjacency (B,N,N) and rewards (B) to host memory, or with
 * SHEP_OUT_DEVICE to caller-owned device memory (e.g. a torch tensor's data_ptr()), as
 * float64 or with SHEP_OUT_F32 float32. */
int shep_get_obs(shep_handle* h, void* dst, int flags);
int shep_get_adj(shep_handle* h, void* dst, int flags);
int shep_get_rewards(shep_handle* h, void* dst, int flags);
/* The three in one copy and one wait (the drop-in env's step): dst, host float64, holds
 * the observation (B,N,4), then the adjacency (B,N,N), then the rewards (B). */
int shep_get_outputs(shep_handle* h, double* dst);
/* The control of the last step (B,N,2) host: shepherd rows u * action_scalar, sheep rows
 * the repulsion (:89). */
int shep_get_controls(shep_handle* h, double* dst);
int shep_sync(shep_handle* h);

/* Per-env random streams: NumPy's legacy RandomState (MT19937), a key of 624 words and a
 * position in [0, 624] per env, as RandomState.get_state() gives them. env = -1: every
 * env (keys (B,624), pos (B)); else one env's (624) and (1). shep_get_rng: GF_ESTATE for an
 * env whose stream was never seeded (SHEP_RESET_SEED) or set. */
int shep_set_rng(shep_handle* h, int env, const uint32_t* keys, const int32_t* pos);
int shep_get_rng(shep_handle* h, int env, uint32_t* keys, int32_t* pos);

typedef struct shep_reset_config {
  double r_max;          /* self.r_max = r_max_init * sqrt(N) (:38-39); finite and > 0 */
  double goal_offset[2]; /* self.goal_offset (:42)                                     */
} shep_reset_config;
#define SHEP_RESET_SEED          0x1 /* seed env b as RandomState(seed + b) first (else its
                                        stream continues)                                 */
#define SHEP_RESET_ZERO_HEADINGS 0x2 /* headings := 0 (else kept, as reset() :187-202
                                        keeps x[:, 2]; a handle that never had a state
                                        resets as from the all-zero state)                */
/* reset() :187-202 of the selected envs (env_mask (B) bytes, NULL = all) in one launch,
 * each from its own stream in the reference's order: length[i] = sqrt(0 + r_max * d) for
 * all N agents, then angle[i] = pi * (0 + 2 * d), d NumPy's random_sample double of two
 * consecutive words; x = length * cos(angle) + goal_offset[0], y = length * sin(angle) +
 * goal_offset[1]. A reset takes 4N words. Lengths, angles and the stream afterwards are
 * NumPy's bit for bit; cos / sin are the device's. The launch also writes the observation,
 * adjacency and reward of the new state (as shep_observe) and zeroes the selected envs'
 * episode step counts; the handle then has a state and an observation and no controls.
 * Unselected envs keep state, outputs and stream; a mask that selects none does nothing.
 * Asynchronous on the handle's stream. Before any device work: GF_EINVAL for a null handle
 * or config, unknown flags, r_max not finite or not > 0, or (SHEP_RESET_SEED) seed +
 * n_envs not fitting in 32 bits; GF_ESTATE for continuing the stream of a selected env
 * that was never seeded or set. */
int shep_reset_device(shep_handle* h, const shep_reset_config* rc, uint64_t seed, const uint8_t* env_mask, int flags);

/* The envs' episode step counts (B): every stepping call advances them (shep_step 1,
 * shep_step_expert and shep_expert_rollout n), shep_set_state and shep_reset_device (for
 * its selected envs) zero them, and so does a reset inside shep_expert_rollout. */
int shep_get_episode_steps(shep_handle* h, int32_t* out);

typedef struct shep_rollout_records { /* every pointer may be NULL: not recorded */
  void* obs;         /* (K,B,N,4) after every record_every-th step, K = n_steps / record_every */
  void* adj;         /* (K,B,N,N)                                                             */
  void* actions;     /* (n_steps,B,n_shepherds,2) controller() of the state before the step,
                        before action_scalar                                                  */
  double* rewards;   /* (n_steps,B)                                                           */
  uint8_t* done;     /* (n_steps,B) 1 on an episode's last step                               */
  int32_t* n_resets; /* (B) resets done inside this launch                                    */
} shep_rollout_records;
#define SHEP_REC_DEVICE 0x4 /* the records are caller-owned device memory (stream-ordered,
                               shep_sync); else host arrays, and the call waits             */
#define SHEP_REC_F32    0x8 /* obs, adj and actions are float32 (else float64)             */
/* n_steps of u = controller(); step(u) in one launch, as shep_step_expert, recording on
 * the way. episode_length = L > 0 runs the reference driver's loop `reset(); for t in
 * range(L): u = controller(); step(u)` episode after episode: an env whose episode step
 * count reaches L with a step has done = 1 there (rewards holds that step's reward), and
 * its wave or workgroup then performs shep_reset_device's reset on the env's continued
 * stream inside the launch (headings kept, count to 0). The row recorded after that step
 * is the reset state's, so (obs before the call, actions[0]) and (obs[t], actions[t+1])
 * are (observation, expert action) pairs across episode ends, and the terminal
 * observation is not recorded. For every env the launch equals, bit for bit in state,
 * outputs, last controls (the last step's, also when a reset followed it), streams and
 * counts, the host-paced loop `shep_step(SHEP_U_EXPERT); if count >= L:
 * shep_reset_device(mask = {b})`; launches chain. L = 0 never resets. Before any device
 * work: GF_EINVAL for n_steps < 1, record_every < 1 or not dividing n_steps, L < 0, L > 0
 * with a null or invalid rc, unknown flags; GF_ESTATE without a state, or with L > 0 and
 * an env whose stream was never seeded or set. */
int shep_expert_rollout(shep_handle* h, int n_steps, int record_every, int episode_length, const shep_reset_config* rc,
                        const shep_rollout_records* rec, int flags);

/* Diagnostics ---------------------------------------------------------------- */
const char* fe_last_error(void);
int fe_abi_version(void);
/* Average device time (ms) of the step kernel, measured with HIP events on the
 * handle's stream (bench roofline). enable >= 1 starts timing every enable-th launch
 * (events keep a sampled launch from overlapping its neighbours); 0 reads and stops;
 * -1 reads and keeps timing. With split steps (fe_set_streams, 2 by default) the
 * result is the device time of the whole window since enable divided by the steps in
 * it, and `launches` counts steps (each two concurrent half-batch launches). */
int fe_kernel_timing(fe_handle* h, int enable, double* avg_ms, int64_t* launches);
/* Launches per step: 2 (default) sends envs
 * [0, ceil(B/2)) to the handle's stream and the rest to a second stream; each half
 * depends only on its own previous step, so one launch's ramp and tail overlap the
 * other's body. Every other call first orders the handle's stream after both halves,
 * so getters and fe_sync see whole steps. A step follows as one launch when other
 * work was enqueued on the handle since the previous step. */
int fe_set_streams(fe_handle* h, int n);
/* Order the handle's stream after all of its outstanding work (enqueue only, no host
 * wait): for zero-copy consumers that enqueue on fe_buffers.stream after fe_step. */
int fe_join(fe_handle* h);
/* The same for cov_step_kernel on a Coverage handle (on a handle that hides nodes, the
 * step kernel and the hidden pass behind it). */
int cov_kernel_timing(cov_handle* h, int enable, double* avg_ms, int64_t* launches);
/* Diagnostics for roofline work: what = 0/1 times `reps` launches of a float4
 * plain/non-temporal fill of the network buffer (the write-bandwidth ceiling).
 * what = 0x10000 | bits (16 bits) sets ablation switches on later step launches
 * (0x10000 clears) in the diagnostic build only (make diag, -DGF_DIAG); the product
 * library returns GF_EINVAL for it and never reads an environment variable. */
int fe_diag(fe_handle* h, int what, int reps, double* avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* GYMFLOCK_H */
