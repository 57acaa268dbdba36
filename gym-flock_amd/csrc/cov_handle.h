// struct cov_handle and the internal calls between the three files of the Coverage C-ABI
// (include/gymflock.h, cov_* functions): cov_capi.hip (handle lifecycle, setters and
// getters, wire formats, streams, timing, hidden nodes), cov_maps_capi.hip (targets, maps,
// the occupancy pool) and cov_step_capi.hip (time matrices, resets, steps, experts).
#pragma once
#include <vector>

#include "capi_common.h"
#include "coverage_internal.h"

struct cov_handle {
  cov_config cfg{};
  hipStream_t stream = nullptr;
  // Split steps as in fe_handle: envs [0, ceil(B/2)) step on `stream`, the rest on
  // `stream2`; each half depends only on its own previous step, every other call first
  // makes `stream` wait for `stream2`.
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_s2 = nullptr, ev_main = nullptr;
  // launches per step (cov_set_streams): 0 = auto, the greedy steps (COV_ACTIONS_GREEDY)
  // split in two, every other step one launch; 1; 2
  int nsplit = 0;
  bool s2_pending = false, main_dirty = true;
  bool other_work = true;  // non-step work since the last step: next step is one launch
  hipEvent_t tw[2] = {nullptr, nullptr};
  int64_t tw_steps = 0;
  gf::CovArgs a{};
  int32_t* ntg = nullptr;
  double* tgt = nullptr;
  int32_t* actions = nullptr;
  int32_t* start = nullptr;
  uint8_t* visited0 = nullptr;
  int32_t* envsel = nullptr;
  int* err = nullptr;
  std::vector<int> ntg_host;
  bool has_graph = false, has_state = false;
  // greedy expert (allocated on first use)
  uint16_t* tm_cost = nullptr;
  uint8_t* tm_cost8 = nullptr;   // uint8 copy of the cost rows (envs that fit), greedy step
  uint8_t* tm_wide = nullptr;    // (B) 1: the env's matrix needed uint16 entries
  std::vector<uint8_t> tm_wide_host;
  int16_t* tm_prevT = nullptr;
  uint16_t* tm_glist = nullptr;  // greedy lists (B,Tmax,gstride), Tmax <= kGreedyListMaxT
  uint16_t* tm_glen = nullptr;   // (B,Tmax)
  int gstride = 0;
  uint8_t* tm_flags = nullptr;
  size_t tm_flags_bytes = 0;     // grown when a plan takes narrower tiles (more chunks per env)
  int32_t* tm_sched_scratch = nullptr;  // the schedule kernel's edges and levels when they exceed the LDS
  size_t tm_sched_scratch_words = 0;
  int tm_plan_s = 0;             // cov_set_tm_plan: sources per wave (0: the largest that fits)
  int tm_plan_global = 0;        //   1: the schedule's edges and levels in the global scratch
  uint8_t* needs_random = nullptr;
  int32_t* tm_envsel = nullptr;
  uint32_t* tm_sched = nullptr;
  int32_t* tm_lev = nullptr;  // (B, 4 * Tmax + 2): the schedule levels' slot offsets
  int32_t* tm_nslots = nullptr;
  int32_t* tm_nlev = nullptr;
  uint8_t* tm_overflow = nullptr;
  std::vector<int> n_motion_host;
  std::vector<char> tm_valid;
  bool tm_ready = false;           // every env's time matrix (and greedy lists) is current
  int64_t tm_wide_envs = 0;  // envs whose matrix needed uint16 entries (diagnostics)
  // wire formats: scratch for host-bound outputs (not zero-filled), graph-tuple offsets
  unsigned char* scratch = nullptr;
  size_t scratch_bytes = 0;
  int64_t* goff = nullptr;
  // step-kernel timing (cov_kernel_timing): HIP events around every stride-th launch
  bool timing = false;
  int timing_stride = 1;
  int64_t timing_count = 0;
  std::vector<hipEvent_t> ev;
  size_t ev_used = 0;
  int32_t* herr = nullptr;  // cov_step_host: page-locked per-env copies of the error word
  // cov_step_host: the launch's completion flag (done_flag.h): device counter, page-locked
  // word, its mapped address
  int32_t* fin_cnt = nullptr;
  int32_t* fin_host = nullptr;
  int32_t* fin_dev = nullptr;
  int32_t fin_seq = 0;
  // COV_GREEDY_RNG: every env's np_random stream (cov_set_rng; allocated on first use)
  uint32_t* mt_key = nullptr;  // (B,624)
  int32_t* mt_pos = nullptr;   // (B)
  // cov_generate_maps (allocated on first use): each env's map stream (the reference's
  // global np.random), its cities, the kernel's per-env outputs, and the lattice of the
  // last map configuration (the same for every env)
  uint32_t* map_key = nullptr;   // (B,624)
  int32_t* map_pos = nullptr;    // (B)
  bool map_seeded = false;
  double* map_cities = nullptr;  // (B, kMapMaxCities, 2)
  int32_t* map_nraw = nullptr;   // (B)
  int32_t* map_status = nullptr; // (B)
  double2* lat = nullptr;        // (L)
  int32_t* lat_cell = nullptr;   // (L)
  int32_t* lat_grid = nullptr;   // (NI * NJ)
  int lat_L = 0, lat_NI = 0, lat_NJ = 0;
  double lat_key[5] = {0, 0, 0, 0, 0};  // x_min, x_max, y_min, y_max, spacing of `lat`
  // cov_load_occupancy: the target pool of an occupancy grid, shared by every env
  cov_occupancy_config occ{};
  bool pool_loaded = false;
  int pool_n = 0, pool_n0 = 0, pool_n1 = 0, pool_K = 0;
  uint8_t* occ_grid = nullptr;      // (n0 * n1)
  int32_t* pool_cellmap = nullptr;  // (n0 * n1) cell -> pool point or -1
  int32_t* pool_rawcell = nullptr;  // (kPoolCap) the pool kernel's scratch
  double2* pool_raw = nullptr;      // (kPoolCap)
  double2* pool_xy = nullptr;       // (kPoolCap) the pool
  int32_t* pool_cell = nullptr;     // (kPoolCap) each pool point's cell
  double* pool_info = nullptr;      // (6) min_xy, max_xy, subgraph_size
  int32_t* pool_counts = nullptr;   // (3)
  int32_t* sub_tries = nullptr;     // (B) cov_generate_submaps: tries consumed
  std::vector<double> pool_host;    // (pool_n, 2)
  double pool_info_host[6] = {0, 0, 0, 0, 0, 0};
  // cov_set_hidden: the hidden-node observation (coverage_hidden.hip), rewritten by
  // cov_hidden_kernel after every pass that makes an observation
  bool hidden = false;
  uint8_t* discovered = nullptr;  // (B,M)
  float* hnodes = nullptr;        // (B,M,4)
  int32_t* hsenders = nullptr;    // (B,4M)
  uint8_t* gmask = nullptr;       // (B,Tmax) visited | !discovered
  int32_t* ngmask = nullptr;      // (B)
  int32_t* hnkeep = nullptr;      // (B) hsenders slots that are not -1
  // cov_reset_device (allocated on first use): the selected envs, the same with the envs
  // that are not reset struck out (-1), each env's start region, status bits and region size
  int32_t* rs_envs = nullptr;     // (B)
  int32_t* rs_ok = nullptr;       // (B)
  uint8_t* rs_region = nullptr;   // (B,Tmax)
  int32_t* rs_status = nullptr;   // (B)
  int32_t* rs_nregion = nullptr;  // (B)
  int32_t* rs_start_c = nullptr;  // (B,R) the selected envs' rows by position in the list
  uint8_t* rs_visited_c = nullptr;  // (B,Tmax)
  uint8_t* rs_region_c = nullptr;   // (B,Tmax)
  // the configuration of the last cov_generate_maps call that drew its cities from the map
  // streams (COV_RESET_NEW_MAPS draws the next maps with it)
  cov_map_config map_cfg{};
  bool map_cfg_set = false;
  // owns every device buffer above and those of `a`; last, so the fields a step reads stay together
  gf::DeviceBuffers mem;
};

// Internal to the library: hidden, so none of these is one of its dynamic symbols.
#pragma GCC visibility push(hidden)
namespace gf {

constexpr const char* kHiddenFused =
    "a handle with hidden nodes has no fused expert (the step kernel reads the visited flags, not the expert's "
    "visited-or-undiscovered mask): take the actions from cov_controller_greedy, then cov_step";

// `stream` behind what `stream2` still holds. Inline: every cov_step passes through it.
static inline int join_s2(cov_handle* h) {
  if (h->s2_pending) {
    GF_HIP(hipEventRecord(h->ev_s2, h->stream2));
    GF_HIP(hipStreamWaitEvent(h->stream, h->ev_s2, 0));
    h->s2_pending = false;
  }
  return GF_OK;
}

// cov_capi.hip
// Every call but cov_step: the device, `stream` after all outstanding work, and what
// it enqueues ordered before the next second-half step.
int use(cov_handle* h);
int check_err(cov_handle* h);  // read and clear the device error bits; translate to a status
int copy_out(cov_handle* h, void* dst, const void* src, size_t bytes);  // to the host, enqueued (null dst: nothing)
// Device scratch of at least `bytes` (grown on demand, reused across calls, not filled).
int scratch(cov_handle* h, size_t bytes, unsigned char** out);
// The same for n host-bound records of bytes[k] bytes (0: not wanted), each 16-byte
// aligned: rec[k] is record k's device address, or nullptr.
int scratch_records(cov_handle* h, int n, const size_t* bytes, unsigned char** rec);
CovHiddenArgs hidden_args(const cov_handle* h);
// Hidden handles (else nothing), on the handle's stream: discovered := robots only for the
// n envs listed on the device (nullptr: every env); every env's hidden observation from
// the ordinary one.
int hidden_reset(cov_handle* h, const int32_t* envs, int n);
int hidden_pass(cov_handle* h);

// cov_maps_capi.hip: cov_generate_maps / cov_generate_submaps for the envs of `sel`
// (ascending; the outputs and the given draws by position in sel, given cities and
// cities_out rows of a contiguous range from sel[0]), one launch of each kernel. The
// public calls have checked mc, flags and the given arrays; cov_reset_device passes none.
int generate_maps_sel(cov_handle* h, const cov_map_config* mc, const std::vector<int32_t>& sel, uint64_t map_seed,
                      const double* cities, int flags, int32_t* n_targets_out, int32_t* status_out,
                      double* cities_out);
int generate_submaps_sel(cov_handle* h, const std::vector<int32_t>& sel, uint64_t map_seed, const double* draws,
                         int n_draws, int flags, int32_t* n_targets_out, int32_t* status_out, int32_t* tries_out);

// cov_step_capi.hip
int ensure_time_matrix(cov_handle* h);  // of every env whose graph changed since they were last built
int ensure_rng_streams(cov_handle* h);  // the envs' np_random streams (mt_key, mt_pos), allocated on first use

}  // namespace gf
#pragma GCC visibility pop
