// Internal interface between the C-ABI (capi.hip) and the kernels (flock_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "done_flag.h"

namespace gf {

// Ablation switches (StepArgs / KnnArgs .diag, timing experiments that give wrong
// outputs) exist only in the diagnostic build (make diag: -DGF_DIAG); the product build
// compiles every such branch out.
// -DGF_CT_ABLATE=<mask>: the same switches as compile-time constants, for register
// studies (scripts/vgpr_phases.sh: each phase compiled out, -Rpass-analysis per build).
#if defined(GF_CT_ABLATE)
#define GF_ABLATE(args, bits) ((static_cast<unsigned long long>(GF_CT_ABLATE) & (bits)) != 0)
#elif defined(GF_DIAG)
#define GF_ABLATE(args, bits) (((args).diag & (bits)) != 0)
#else
#define GF_ABLATE(args, bits) false
#endif

constexpr int kThreads = 256;   // 4 wave64s per workgroup
constexpr int kTileMax = 1024;      // max agents per LDS tile (32 KiB of float64 state)
constexpr int kTileDefault = 512;   // default tile (measured best, see step_tile)
constexpr size_t kStepLdsPlainFloor = 24 * 1024;  // plain step: 6 workgroups per CU, not 7
constexpr int kKnnLdsMax = 4096;    // kNN stages the env's positions in LDS up to this N
constexpr int kKnnGridCells = 2048; // kNN: cells of the per-env uniform grid (at most)
constexpr int kInlineRimU = 4;      // fused kNN inline rim scan: columns in flight per lane
constexpr int kStoreTab = 16;      // network rows: float4 table entries per wave (one per nibble)
constexpr int kNetDeltaBatch = 64;  // delta network store: record words a wave compares at a time
constexpr size_t kNetDeltaLds = 4 * kNetDeltaBatch * 8;  // their changed bits in LDS, per wave
// a batch with more dirty groups than this (of 256) takes the row loop instead of the
// compacted drain (-DGF_NET_COMPACT_MAX for A/B; DESIGN.md §4, "Compacted drain")
#ifndef GF_NET_COMPACT_MAX
#define GF_NET_COMPACT_MAX 128
#endif
constexpr int kNetCompactMax = GF_NET_COMPACT_MAX;
constexpr int kStepInlineRim = 2;  // fused kNN: unranked rows a wave ranks itself (more: rim kernel)
constexpr int kStepExactKnnMax = 128;  // fused kNN: envs up to this size are ranked exactly in
                                       // the step (KX: one tile in LDS, no rim kernel)
constexpr int kStepExactKnnMaxOneEnv = 192;  // the same for a handle of one env (the drop-in
                                             // step: its tile then holds the whole env); beyond
                                             // it the per-row scan costs more than the rim
                                             // kernel it saves (profiles/r05/ab_dropin_exact_one_env.txt)
constexpr int kKnnRimGrid = 256;     // rim kNN: workgroups walking the flagged blocks
constexpr int kKnnRimHalfGrid = kKnnRimGrid / 2;  // the same per half-batch launch
constexpr int kKnnFewSlow = 16;     // kNN: up to this many rows to scan per workgroup are
                                    // scanned wave-cooperatively from L2, more through the grid
// kNN LDS: positions (16 B per agent), the grid's cell offsets, agent indices by cell
constexpr size_t knn_lds_bytes(int N) {
  return (size_t)N * 16 + (size_t)(kKnnGridCells + 1) * 4 + (((size_t)N * 2 + 15) / 16) * 16;
}

// One batched hot-path launch. Pointers are device pointers; all per-env arrays
// are [B][N][...] contiguous.
struct StepArgs {
  const double* x_in;     // (B,N,4) state before the step
  double* x_out;          // (B,N,4) state after the step (DYN only)
  const void* u;          // (B,N,2) float or double actions (DYN only)
  float* state_values;    // (B,N,6) or nullptr
  float* network;         // (B,N,N) or nullptr
  double* ctrl_out;       // (B,N,2) or nullptr (CTRL only)
  double* reward;         // (B) or nullptr
  double* reward2;        // (B) or nullptr: a second copy (fe_step_host's page-locked array)
  double dt, action_scalar, cr, cr2;
  float dt_f, as_f;
  int N, B;
  int R;                  // rows per workgroup (power of two, 4..64)
  int T;                  // agents per LDS tile (multiple of 64)
  int bpe;                // workgroups per env = ceil(N / R)
  int mean_pooling, centralized;
  int prefetch;           // tiled step issues each tile's loads one tile ahead (T <= 512)
  int store_fast;         // network rows by the fast bit-extract loop (N % 1024 == 0)
  int u_inline;           // u is a host pointer: its B*N actions travel in the kernel arguments
                          // (StepArgsU; one env of one tile, <= kUInlineBytes)
  int diag;               // ablation switches, read only by the diagnostic build (GF_ABLATE):
                          // 2 skip feature pass,
                          // 4 non-temporal network stores, 8 skip pass 1 (bits are left
                          // unwritten: timing only), 16 skip tile loads (timing only),
                          // 64 / 128 generic / fast network store loop (A/B), 256 no
                          // per-row outputs, 512 no reward, 1024 constant network rows
                          // (timing only), 8192 plain XCD remap for the plain step (A/B)
  // Flocking variants (flocking_leader/obstacle/stoch.py). variant == 0 keeps the
  // FlockingRelative path untouched; otherwise the fields below apply (tiled kernel).
  int variant;
  int n_frozen;           // agents [0,n) ignore actions (their mask is 0)
  int n_vel_zero;         // pairs touching agents [0,n) have zero velocity difference
  double u_scale;         // the step's action multiplier (action_scalar is the controller's)
  double u_clip;          // clip actions to +-u_clip before scaling; <= 0: none
  double x_scale;         // state multiplied before / divided after the update
  double ctrl_clip;       // controller output clip; <= 0: none
  float us_f, uc_f;       // float32 copies of u_scale, u_clip
  const double* dt_env;   // (B) per-env dt of this step, or nullptr (dt)
  uint64_t* adj_bits;     // (B,N,Wn) packed adjacency or nullptr
  int32_t* degree_out;    // (B,N) degrees or nullptr
  // Flocking-v0 k-nearest selection fused into the feature pass (kStepFusedK neighbours):
  // rows the step can rank exactly get idx + obs; the others get idx[row*K] = -1 and
  // are finished by flock_knn_kernel in rim mode. Key of a ranked pair:
  // (min(floor(r2 * knn_qscale / Tr), knn_qmax) << knn_jbits) | j (see the kernel).
  int32_t* knn_idx;       // (B,N,K) or nullptr: no fused selection
  float* knn_obs;         // (B,N,4K)
  float* knn_r2;          // (B,N) k-th nearest r2 of the state two steps back (0: none),
                          // replaced by this state's for the rows ranked here
  uint8_t* knn_rimflag;   // (B, ceil(N/256)): set for each 256-row block holding a row
                          // left to the rim kNN (its workgroups read only this byte)
  double knn_qscale;      // 2^qbits
  unsigned knn_qmax;      // 2^qbits - 2
  double knn_qmaxd;       // the same as a double (compared with r2 * scale)
  int knn_jbits;          // bits of the agent index (qbits = 32 - jbits)
  int knn_exact;          // the handle's fused selection is exact in the step (step_knn_exact)
  DoneFlag fin;           // drop-in launch: the grid's completion flag (done_flag.h)
  // Delta network store (the plain step into the handle's own buffer, N % 4 == 0; set by
  // the C-ABI's timed_launch only): the record of what `network` holds. Row i holds
  // net_val[i] at the set bits of net_bits[i] and +0.0f elsewhere; the launch stores only
  // the groups (net_delta.h) whose content changes and brings the record up to date.
  uint64_t* net_bits;     // (B,N,Wn) or nullptr: every row stored in full, no record kept
  float* net_val;         // (B,N)
  int net_force;          // store every group and write the record (its content is not valid)
};

// The drop-in step's actions passed in the kernel arguments (fe_step_host, one env of up
// to kUInlineBytes of actions: 384 agents in float32, 192 in float64)
constexpr int kUInlineBytes = 3072;
struct StepArgsU {
  StepArgs a;
  alignas(16) unsigned char u[kUInlineBytes];
};

constexpr int kStepFusedK = 7;  // Flocking-v0's n_neighbors (flocking.py:9)

struct KnnArgs {
  const double* x;        // (B,N,4) current state
  int32_t* idx;           // (B,N,K)
  float* obs;             // (B,N,4K)
  int N, B, K;
  const uint64_t* adj_bits;  // (B,N,Wn) adjacency of x from the step, or nullptr
  const int32_t* degree;     // (B,N) with adj_bits
  int rim;                   // only rows the fused step left unranked (idx[row*K] < 0)
  float* r2k;                // (B,N) or nullptr: each ranked row's k-th nearest r2
  uint8_t* rimflag;          // rim mode: (B, ceil(N/256)) blocks the step marked (cleared here)
  int grid_cap;              // rim mode: workgroups (0: kKnnRimGrid)
  int diag;                  // ablation (fe_diag bits << 12, apart from the step's): 0x4000 no ranking on the neighbour path, 0x8000 no neighbour path,
                             // 0x1000 grid built but no search, 0x2000 no grid / scan, 0x0800 no outputs
  DoneFlag fin;              // drop-in launch: the grid's completion flag (done_flag.h)
};

struct StatsArgs {
  const double* x;        // (B,N,4)
  double* vel_diffs;      // (B,N)
  double* min_dists;      // (B,N)
  int32_t* degree;        // (B,N) neighbours with r2 < comm_radius^2
  double cr2;
  int N, B;
};

// reset() on the device (flock_reset.hip; flocking_relative.py:156-192): one workgroup per
// selected env draws candidates from the env's MT19937 stream until one passes the
// reference's acceptance test, at most max_tries of them.
constexpr int kResetMaxN = 1024;        // rejection mode: positions and velocities in LDS
constexpr int kResetMaxTries = 65536;
struct ResetArgs {
  int n_sel;
  const int32_t* envs;    // (n_sel) env of each workgroup, or nullptr: envs 0..n_sel-1
  int N;
  int reject;             // 0: keep the first draw, no pair test (the synthetic init)
  int seeded;             // stream b := RandomState(seed0 + b) first; else continued
  uint32_t seed0;
  double r_max, v_max, v_bias;
  double min_dist, cr2;   // cr2: comm_radius * comm_radius as the host rounds it
  int min_degree, max_tries;
  double* x;              // (B,N,4) the state buffer written (selected envs only)
  uint32_t* mt_key;       // (B,624) each env's stream
  int32_t* mt_pos;        // (B) in [0, 624]
  int32_t* tries;         // (B) out: candidates drawn
  uint8_t* status;        // (B) out: FE_RESET_EXHAUSTED
  int32_t* has_gauss;     // (B) the streams' cached Gaussian (flock_dt_noise.hip): cleared
  double* gauss;          // (B) for the envs a seeded reset selects
};
size_t reset_lds_bytes(int N, bool reject);
hipError_t launch_reset(const ResetArgs& a, hipStream_t s);

// flock_dt_noise.hip: n consecutive np.random.normal(mean, sigma) per env from the env's
// stream (legacy_gauss with its cache), dt_steps[t * B + b] the t-th of env b.
struct DtNoiseArgs {
  int B, n;
  double mean, sigma;
  uint32_t* mt_key;       // (B,624)
  int32_t* mt_pos;        // (B) in [0, 624]
  int32_t* has_gauss;     // (B) RandomState.get_state()[3]
  double* gauss;          // (B) RandomState.get_state()[4]
  double* dt_steps;       // (n,B) out
};
hipError_t launch_dt_noise(const DtNoiseArgs& a, hipStream_t s);

// flock_dt_noise.hip: the variants' resets (FE_VRESET_*), one wave per selected env. Leader
// runs after launch_reset on the same envs and only overrides the leaders' velocities.
constexpr int kVResetLeader = 1, kVResetTwoFlocks = 2, kVResetObstacle = 3;
struct VResetArgs {
  int kind;
  int n_sel;
  const int32_t* envs;    // (n_sel) or nullptr: envs 0..n_sel-1
  int N;
  int n_special;          // leaders / obstacles: agents [0, n_special)
  int seeded;             // stream b := RandomState(seed0 + b) first (never with Leader: its
  uint32_t seed0;         // rejection reset has seeded the stream already)
  double v_max, v_bias;
  double* x;              // (B,N,4)
  uint32_t* mt_key;
  int32_t* mt_pos;
  int32_t* has_gauss;
  double* gauss;
  int32_t* tries;         // (B) out: 1 (TwoFlocks, Obstacle)
  uint8_t* status;        // (B) out: 0 (TwoFlocks, Obstacle)
};
hipError_t launch_vreset(const VResetArgs& a, hipStream_t s);

// The closed-loop expert rollout (flock_rollout.hip): n_steps of u = controller();
// step(u) in one launch, one workgroup (of up to 1024 threads) per env that keeps the env's
// state in LDS.
constexpr int kRolloutMaxN = 256;  // every size at which the reference's reset() accepts a draw
struct RolloutArgs {
  // The constants, variant switches and per-env dt of a step (base_args), and the handle's
  // buffers: x_in / u (float64) the state and its controller output before the first step;
  // x_out, ctrl_out, state_values, adj_bits, degree_out and reward are written by the last
  // step (any may be nullptr).
  StepArgs s;
  int n_steps;
  int record_every;       // >= 1: record step t when (t + 1) % record_every == 0
  // records (K = n_steps / record_every), each (K,B,N,.) or nullptr
  double* rec_x;          // (K,B,N,4)
  float* rec_sv;          // (K,B,N,6)
  uint64_t* rec_bits;     // (K,B,N,Wn)
  int32_t* rec_deg;       // (K,B,N)
  double* rec_ctrl;       // (K,B,N,2)
  double* rec_rewards;    // (n_steps,B): every step's
  // (n_steps,B) or nullptr: step t of env b integrates with dt_steps[t * B + b] instead of
  // the launch's dt (variant launches only: fe_set_dt_noise)
  const double* dt_steps;
};
int rollout_chunk_bits(int N);  // columns per pass-2 thread: 16, 32, 64 for N <= 64, 128, 256
hipError_t launch_rollout(const RolloutArgs& a, hipStream_t s);

// The DAgger rollout (flock_policy_rollout.hip): the expert rollout's step, driven per step
// by the expert or by a small per-agent network over delayed aggregation features.
constexpr int kPolicyMaxTaps = 4, kPolicyMaxLayers = 3, kPolicyMaxWidth = 64;
// The network as the kernel keeps it in LDS (float32). A hidden layer of n_in inputs and
// w_out outputs gives each of a row's four threads Pw = w_out / 4 consecutive outputs,
// padded to PS = 4 * ceil(Pw / 4) so that a thread reads its weights of one input as float4s:
// weights [n_in][4][PS] (entry [i][q][m] = weight[q * Pw + m][i], 0 for m >= Pw), then the
// biases [4][PS]. The last layer (2 outputs): weights [n_in][4] (entry [i][o], 0 for
// o >= 2), then 4 biases.
struct PolicyNet {
  const float* image;     // device: the layers in the layout above, n_floats of them
  int n_floats;
  int n_layers, n_taps;
  int width[kPolicyMaxLayers + 1];
  int off_w[kPolicyMaxLayers], off_b[kPolicyMaxLayers];  // float offsets into image
  float clip;             // > 0: the two outputs are clipped to [-clip, clip]
};
// Floats of the image of a network of these widths, and the offsets into it (any may be
// nullptr); what the kernel reads past a layer's real outputs is zero-filled by the packer.
int policy_image_floats(int n_layers, const int* width, int* off_w, int* off_b);
// weight[l] (width[l+1], width[l]) row-major and bias[l] into `image` (policy_image_floats)
void policy_pack_image(int n_layers, const int* width, const float* const* weight, const float* const* bias,
                       float* image);
struct PolicyRolloutArgs {
  // As the expert rollout's (dt_steps unused). r.s.state_values is also read: tap 0 of the
  // state before the first step.
  RolloutArgs r;
  PolicyNet net;
  float* taps;            // (B,N,n_taps-1,6) taps 1.. of the state before the first step; the
                          // last step writes the final state's (nullptr with n_taps == 1)
  const uint8_t* mask;    // (n_steps,B) used_expert of every step, or nullptr: mask_const
  int mask_const;
  float* rec_agg;         // (K,B,N,n_taps,6)
  float* rec_policy;      // (K,B,N,2)
  double* rec_applied;    // (n_steps,B,N,2)
  uint8_t* rec_used;      // (n_steps,B)
};
// The kernel's dynamic LDS: the one expression of the host's guard and of the launch.
size_t policy_rollout_lds_bytes(int N, int n_taps, int image_floats);
constexpr size_t kPolicyLdsMax = 80 * 1024;  // two workgroups per CU (160 KB)
hipError_t launch_policy_rollout(const PolicyRolloutArgs& a, hipStream_t s);

// flock_dt_noise.hip: n consecutive random_sample() doubles per env from the env's stream,
// mask[t * B + b] = (the t-th of env b) < beta. The cached Gaussian is left alone.
struct MixMaskArgs {
  int B, n;
  double beta;
  uint32_t* mt_key;       // (B,624)
  int32_t* mt_pos;        // (B) in [0, 624]
  uint8_t* mask;          // (n,B) out
};
hipError_t launch_mix_mask(const MixMaskArgs& a, hipStream_t s);

// Launch-geometry helpers shared by host and tests.
int step_rows_per_block(int N);
int step_tile(int N);
size_t step_lds_bytes(int N, int R, int T, bool ctrl, bool knn);

hipError_t launch_step(const StepArgs& a, bool dyn, bool u_f64, bool ctrl, hipStream_t s);

// Whether a step of this geometry can carry the fused k-nearest selection (K ==
// kStepFusedK, no variant, no tile prefetch, at least K word-slices per row).
bool step_fused_knn_ok(int N, int R, int K, bool variant, bool prefetch);
// Whether the fused selection of a handle of B envs of N agents (tile T) ranks every row
// exactly in the step (the KX instantiation: one tile, N <= kStepExactKnnMax, or one env of
// up to kStepExactKnnMaxOneEnv agents): no rim kernel follows.
bool step_knn_exact(int N, int T, int B);
hipError_t launch_knn(const KnnArgs& a, hipStream_t s);
hipError_t launch_stats(const StatsArgs& a, hipStream_t s);
// per env: mean vel_diffs, mean min_dists of launch_stats' outputs -> out (B,2)
hipError_t launch_stats_summary(const StatsArgs& a, double* out, hipStream_t s);
// Diagnostic: stream `bytes` of float4 stores into p (nt = non-temporal), the
// write-bandwidth ceiling of the network buffer on this device.
hipError_t launch_fill(void* p, size_t bytes, bool nt, hipStream_t s);

}  // namespace gf
