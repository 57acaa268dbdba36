// struct fe_handle and the internal calls between the two files of the flocking C-ABI:
// capi.hip (handle lifecycle, state, reset, step, outputs, kNN, stats, timing) and
// flock_comm.hip (the RCCL metrics path).
#pragma once
#include <rccl/rccl.h>

#include <deque>
#include <vector>

#include "capi_common.h"
#include "flock_internal.h"

// Reward ring: the t-th reward-writing launch writes slot t % kRewardSlots. The metrics
// all-gather ships every step written since the previous gather (at most kRewardSlots).
constexpr int kRewardSlots = 64;
// fe_comm_init's bound on the communicator's creation, its shard-size exchange and every
// later wait for a collective
constexpr double kCommInitTimeoutS = 300.0;

struct fe_handle {
  fe_config cfg{};
  hipStream_t stream = nullptr;
  // Split steps: the step's env batch goes out as two launches, envs [0, B0) on
  // `stream` and [B0, B) on `stream2`, so one launch's ramp and tail overlap the other's
  // body (175.8 vs 196.0 us per config-2 step). The halves only depend on
  // their own previous step; `stream` waits for `stream2` (join) before any other work.
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_s2 = nullptr;           // stream2 -> stream join
  hipEvent_t ev_main = nullptr;         // stream -> stream2 ordering
  int nsplit = 2;                       // launches per step (fe_set_streams)
  bool s2_pending = false;              // stream2 holds work `stream` has not waited for
  bool main_dirty = true;               // `stream` holds work stream2 has not waited for
  bool dephase = true;                  // the next split step starts the halves apart (other
                                        // work or a single launch came before it)
  bool other_work = true;               // non-step work was enqueued since the last step:
                                        // the next step goes out as one launch (a split
                                        // step would only wait on it across streams)
  hipEvent_t tw[2] = {nullptr, nullptr};  // split-step timing window (fe_kernel_timing)
  int64_t tw_steps = 0;
  double* x[2] = {nullptr, nullptr};
  int cur = 0;
  void* u = nullptr;                    // (B,N,2) up to float64
  double* ctrl[2] = {nullptr, nullptr};
  int ccur = 0;
  float* sv = nullptr;
  float* net = nullptr;
  // Delta network store (timed_launch): the record of what `net` holds, allocated on first
  // use. Row i of the buffer holds net_val[i] at the set bits of net_bits[i] and +0.0f
  // elsewhere: a description of the buffer, not of the state, so whatever leaves the
  // buffer alone (FE_NO_NETWORK, set_state, reset, set_params, a network sent to
  // page-locked host memory) leaves the record valid.
  uint64_t* net_bits = nullptr;         // (B,N,ceil(N/64))
  float* net_val = nullptr;             // (B,N)
  bool net_record_valid = false;        // the record describes the buffer (host flag)
  int net_store = FE_NET_DELTA;         // fe_set_network_store
  double* reward_ring = nullptr;        // kRewardSlots x B
  int rslot = 0;
  int64_t steps_written = 0;            // reward-writing launches so far (slot = count % slots)
  // kNN outputs, one pair per state buffer: knn_idx[i] / knn_obs[i] belong to x[i], so
  // a fused step (which writes those of its output state) never overlaps the rim kNN of
  // the previous state, and the kread events that guard x[i] guard them too
  int32_t* knn_idx[2] = {nullptr, nullptr};
  float* knn_obs[2] = {nullptr, nullptr};
  // each ranked row's k-th nearest r2 (0: unknown), by state buffer: a fused step reads
  // the one of two states back (complete: the step waits for that state's kNN) to pick
  // the rows it ranks beyond their neighbours, and writes its own
  float* knn_r2[2] = {nullptr, nullptr};
  uint8_t* knn_rimflag[2] = {nullptr, nullptr};  // per state buffer: blocks with rim rows
  double* vel_diffs = nullptr;
  double* min_dists = nullptr;
  int32_t* degree = nullptr;
  int u_resident_f64 = -1;              // dtype of the resident actions (-1: none)
  bool has_state = false, has_ctrl = false, has_obs = false, has_knn = false;
  bool obs_on_host = false;             // the last launch wrote state_values / network to
                                        // host arrays only (fe_step_host): device copies stale
  int R = 0, T = 0, bpe = 0;
  int knn_exact = 0;                    // the fused kNN is exact in the step (gf::step_knn_exact)
  size_t BN = 0;
  int diag = 0;                         // ablation switches (diagnostic build only, fe_diag)
  int prefetch = 0;                     // tile loads one tile ahead (N >= 16 tiles)
  int store_fast[2] = {0, 1};           // fast network store loop: plain step / with controller
  // kernel timing (bench roofline)
  bool timing = false;
  int timing_stride = 1;                // sample every timing_stride-th launch
  int64_t timing_count = 0;
  std::vector<hipEvent_t> ev;
  size_t ev_used = 0;
  hipEvent_t h2d_ev = nullptr;          // completion of the borrowed host-action copy
  // Host actions of split steps (fe_step without FE_U_*): copied on a stream of their own
  // into one of two device buffers, so the copy for step t+1 runs while step t computes;
  // buffer k is rewritten only after both halves of the step that read it (two calls
  // back) have finished (ev_uread), and both halves of its step wait for its copy.
  hipStream_t ustream = nullptr;
  void* ubuf[2] = {nullptr, nullptr};   // (B,N,2) up to float64 each
  hipEvent_t ev_ucopy[2] = {nullptr, nullptr};
  hipEvent_t ev_uread[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  bool uread_live[2] = {false, false};
  int ucur = 0;
  // ring slots a reward gather's staging copy still reads: steps [first, ...) until the
  // copy kernel (on the side stream) has stored `seq` into completion word kWordRing
  struct RingRead {
    int64_t first;
    uint32_t seq;
  };
  // RCCL metrics path (flock_comm.hip). Shards may differ in size: every gathered block is
  // padded to the largest shard (max_envs), rank r's entries past its n_envs are zero.
  struct Metrics {
    ncclComm_t comm = nullptr;
    hipStream_t comm_stream = nullptr;
    int nranks = 1, rank = 0;
    int max_envs = 0;
    std::vector<int32_t> shard_sizes;     // every rank's n_envs (fe_comm_init's exchange)
    double comm_timeout = kCommInitTimeoutS;  // bound on every wait for a collective
    // The step streams never wait on the side stream on the device: a collective stuck on
    // a dead peer (and, through it, everything queued behind it) must not stall the steps.
    // A step about to overwrite a ring slot that a gather's staging copy has not read yet
    // waits for that copy on the host, bounded by comm_timeout (next_reward_slot); normally
    // the copy finished long before (the slot was written kRewardSlots steps ago).
    double* gsend = nullptr;              // kRewardSlots x max_envs: the gathered steps, padded
    double* gather = nullptr;             // nranks x kRewardSlots x max_envs
    hipEvent_t step_ev = nullptr;
    hipEvent_t step_ev2 = nullptr;        // the gather's wait on stream2 (split steps)
    std::deque<RingRead> ring_reads;
    // The side stream's completion words (kWord*): page-locked (mapped, coherent), each
    // stored by a kernel on the side stream with a system-scope release once the work
    // before it is done, and polled by the host instead of querying events; never freed
    // once a communicator was aborted (an abandoned kernel may still store into them)
    uint32_t* stage_done = nullptr;
    uint32_t* stage_done_dev = nullptr;
    uint32_t stage_seq[4] = {0, 0, 0, 0};  // the last sequence number issued per word
    int64_t gathered_upto = 0;            // steps before this one were shipped (or skipped)
    bool ag_issued = false;
    int last_count = 0;
    double* ssend = nullptr;              // (max_envs,2) the stats gather's padded send block
    double* stats_gather = nullptr;       // nranks x max_envs x 2 (fe_allgather_stats)
    bool sg_pending = false;
    // fe_debug_comm_gate: a bounded spin kernel on comm_stream, released by this page-locked
    // flag, stands in for a collective whose peer stopped responding (tests only)
    unsigned* gate_flag = nullptr;
    // fe_debug_comm_state: what the ring-slot reuse and the gathers saw (tests only)
    int32_t dbg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::string comm_lost;                // why the metrics path was torn down (a timed-out wait)
  } met;
  double* stats_sum = nullptr;          // (B,2) get_stats means per env (fe_stats_summary)
  // fe_step_host*: the launch's completion flag (done_flag.h), allocated on first use: the
  // device counter, the page-locked word and its mapped address
  int32_t* fin_cnt = nullptr;
  int32_t* fin_host = nullptr;
  int32_t* fin_dev = nullptr;
  int32_t fin_seq = 0;
  // flocking variant (fe_set_variant / fe_set_dt)
  bool has_variant = false;
  fe_variant var{};
  double* dt_env = nullptr;             // (B) per-env dt
  bool dt_per_env = false;
  // packed output mode (FE_PACKED_NETWORK) and the kNN step's adjacency: two buffers,
  // so a step can write one while the kNN of the previous step reads the other
  uint64_t* adj_bits[2] = {nullptr, nullptr};  // (B,N,Wn)
  int32_t* pdeg[2] = {nullptr, nullptr};       // (B,N)
  int bits_cur = 0;                     // buffer of the latest bits / degrees
  bool has_packed = false;
  // fe_step_expert: the rollout leaves the dense network buffer as it was (its getters
  // return GF_ESTATE until a launch writes it again), and records for host destinations
  // go through a device staging buffer (grow-only)
  bool net_stale = false;
  unsigned char* roll_stage = nullptr;
  size_t roll_stage_bytes = 0;
  // Flocking-v0 pipelining: the kNN of step t runs on kstream, after both halves of
  // step t and beside step t+1. A step that writes the state buffer x[i] (or a bits
  // buffer) an unfinished kNN reads waits for that kNN's event first; every other API
  // call joins kstream into `stream` (use_dev).
  // The fused step's rim kNN (mode 2) is not on kstream: after a split step it goes out
  // as two launches on the step streams themselves, envs [0, B0) behind `stream`'s half
  // and [B0, B) behind stream2's, so each half of the next step follows its own rim by
  // stream order and the halves keep drifting out of phase (Flocking-v0).
  hipStream_t kstream = nullptr;
  hipEvent_t ev_kin[2] = {nullptr, nullptr};  // stream / stream2 -> kstream
  hipEvent_t ev_kjoin = nullptr;              // kstream -> stream
  bool k_pending = false;                     // kstream holds work `stream` has not waited for
  int last_b0 = 0;                            // B0 of the last launch if it was split, else 0
  struct KnnReader {
    hipEvent_t ev = nullptr;                  // the kNN launch on kstream
    bool live = false;
    unsigned bmask = 0;                       // bits buffers it reads
  } kread[2];                                 // by the state buffer x[i] the kNN reads
  // fe_reset_device / fe_set_rng: the envs' MT19937 streams and the reset's outputs,
  // allocated on first use (ensure_rng)
  uint32_t* rng_key = nullptr;                // (B,624)
  int32_t* rng_pos = nullptr;                 // (B)
  int32_t* reset_tries = nullptr;             // (B)
  uint8_t* reset_status = nullptr;            // (B)
  int32_t* reset_envs = nullptr;              // (B) the selected envs of a masked reset
  int32_t* reset_envs_host = nullptr;         // (B) page-locked: the list's upload reads it
  hipEvent_t ev_envs = nullptr;               // that upload (before the list is rewritten)
  std::vector<uint8_t> rng_set;               // (B) the env's stream was seeded or set
  // the streams' cached Gaussian, RandomState.get_state()[3:5] (allocated with the streams)
  int32_t* rng_has_gauss = nullptr;           // (B)
  double* rng_gauss = nullptr;                // (B)
  // fe_set_dt_noise: every step's dt drawn on the device (flock_dt_noise.hip) into dt_steps,
  // which a step reads as its dt_env and a rollout as its per-step table
  bool dt_noise = false;
  double dt_mean = 0.0, dt_sigma = 0.0;
  double* dt_steps = nullptr;                 // (dt_rows,B), grows on demand
  size_t dt_steps_cap = 0;                    // doubles allocated
  int dt_rows = 0;                            // rows the latest draw wrote (0: none yet)
  // fe_set_policy / fe_step_policy: the learner's network as the kernel's LDS image, the
  // taps 1 .. n_taps-1 of the current state's aggregation, and the per-step choices a call
  // with 0 < beta < 1 draws (flock_dt_noise.hip)
  bool has_policy = false;
  gf::PolicyNet policy{};                     // (.image: pol_image)
  float* pol_image = nullptr;                 // grow-only
  size_t pol_image_cap = 0;                   // floats allocated
  float* taps = nullptr;                      // (B,N,n_taps-1,6), grow-only
  size_t taps_cap = 0;                        // floats allocated
  uint8_t* mix_mask = nullptr;                // (n_steps,B), grows on demand
  size_t mix_mask_cap = 0;
};

// capi.hip: each env's get_stats means into stats_sum. Internal like the calls below, but
// it has always been a dynamic symbol of the library: kept, so that list is unchanged.
extern "C" int stats_summary_dev(fe_handle* h);

// Internal to the library: hidden, so none of these is one of its dynamic symbols.
#pragma GCC visibility push(hidden)
namespace gf {

// capi.hip
int use_dev(fe_handle* h);       // every call but the step launches: device, streams joined
int use_dev_step(fe_handle* h);  // the step path: the device only
int d2h(fe_handle* h, void* dst, const void* src, size_t bytes);  // copy to the host, complete
// flock_comm.hip
bool comm_stream_drained(fe_handle* h);
void comm_release(fe_handle* h, bool abort);
int ring_reads_wait(fe_handle* h, int64_t s);  // next_reward_slot's host wait (met.ring_reads)
int stats_send_wait(fe_handle* h);             // stats_summary_dev's (met.sg_pending)

}  // namespace gf
#pragma GCC visibility pop
