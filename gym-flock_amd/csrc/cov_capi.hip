// C-ABI of the Coverage-v0 engine (include/gymflock.h, cov_* functions).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "capi_common.h"
#include "coverage_internal.h"

using gf::dalloc_zero;
using gf::fail;

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
  // wire formats: scratch for host-bound outputs, graph-tuple offsets
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
};

namespace {

int join_s2(cov_handle* h) {
  if (h->s2_pending) {
    GF_HIP(hipEventRecord(h->ev_s2, h->stream2));
    GF_HIP(hipStreamWaitEvent(h->stream, h->ev_s2, 0));
    h->s2_pending = false;
  }
  return GF_OK;
}

// Every call but cov_step: the device, `stream` after all outstanding work, and what
// it enqueues ordered before the next second-half step.
int use(cov_handle* h) {
  GF_HIP(hipSetDevice(h->cfg.device));
  if (int rc = join_s2(h)) return rc;
  h->main_dirty = true;
  h->other_work = true;
  return GF_OK;
}

void cov_release(cov_handle* h) {
  if (!h) return;
  hipSetDevice(h->cfg.device);
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->stream2) hipStreamSynchronize(h->stream2);
  gf::CovArgs& a = h->a;
  void* bufs[] = {h->ntg, h->tgt, a.nbr, a.cnt, a.n_motion, a.xr, a.cur, a.visited, a.nvisited,
                  a.step_counter, a.dirty, h->actions, a.reward, a.done, a.nodes, a.edges, a.senders,
                  a.receivers, a.obs_step, a.axy, a.nrec, h->err, h->start, h->visited0, h->envsel, h->tm_cost, h->tm_cost8, h->tm_wide, h->tm_prevT, h->tm_glist, h->tm_glen,
                  h->tm_flags, h->tm_sched_scratch, h->needs_random, h->tm_envsel, h->tm_sched, h->tm_lev, h->tm_nslots, h->tm_nlev, h->tm_overflow, h->scratch,
                  h->goff, h->mt_key, h->mt_pos, h->map_key, h->map_pos, h->map_cities, h->map_nraw,
                  h->map_status, h->lat, h->lat_cell, h->lat_grid, h->occ_grid, h->pool_cellmap, h->pool_rawcell,
                  h->pool_raw, h->pool_xy, h->pool_cell, h->pool_info, h->pool_counts, h->sub_tries,
                  h->discovered, h->hnodes, h->hsenders, h->gmask, h->ngmask, h->hnkeep,
                  h->rs_envs, h->rs_ok, h->rs_region, h->rs_status, h->rs_nregion,
                  h->rs_start_c, h->rs_visited_c, h->rs_region_c};
  for (void* p : bufs)
    if (p) hipFree(p);
  for (hipEvent_t e : h->ev) hipEventDestroy(e);
  if (h->herr) hipHostFree(h->herr);
  if (h->fin_cnt) hipFree(h->fin_cnt);
  if (h->fin_host) hipHostFree(h->fin_host);
  for (hipEvent_t e : {h->ev_s2, h->ev_main, h->tw[0], h->tw[1]})
    if (e) hipEventDestroy(e);
  if (h->stream) hipStreamDestroy(h->stream);
  if (h->stream2) hipStreamDestroy(h->stream2);
  delete h;
}

// Read and clear the device error bits; translate to a status.
int check_err(cov_handle* h) {
  int err = 0;
  GF_HIP(hipMemcpyAsync(&err, h->err, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  if (!err) return GF_OK;
  GF_HIP(hipMemsetAsync(h->err, 0, sizeof(int), h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  std::string m;
  if (err & 1) m += "a target has more than 4 motion-graph neighbours (coverage.py:257 assert); ";
  if (err & 2) m += "motion edges + 8*n_robots exceed 4*max_nodes (\"Increase MAX_EDGES\", coverage.py:288); ";
  if (err & 4) m += "action outside [0, 4) (coverage.py:189 index); ";
  if (err & 8) m += "greedy next hop is not among the robot's action targets (IndexError at coverage.py:869); ";
  return fail(GF_EINVAL, m);
}

int copy_out(cov_handle* h, void* dst, const void* src, size_t bytes) {
  if (!dst) return GF_OK;
  GF_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
  return GF_OK;
}

// The time-matrix flags (B, nchunk, kcap) for tiles of S sources per wave.
int ensure_tm_flags(cov_handle* h, int S, int kcap) {
  const size_t need = (size_t)h->cfg.n_envs * ((h->a.Tmax + S - 1) / S) * kcap;
  if (need <= h->tm_flags_bytes) return GF_OK;
  if (h->tm_flags) GF_HIP(hipFree(h->tm_flags));
  h->tm_flags = nullptr;
  h->tm_flags_bytes = 0;
  if (int rc = dalloc_zero(&h->tm_flags, need)) return rc;
  h->tm_flags_bytes = need;
  return GF_OK;
}

// Sources per wave for a time-matrix pass over maps of up to t_lds targets: the plan's
// (cov_set_tm_plan, narrowed where this launch's maps need it) or the largest whose tile fits.
int tm_sources(const cov_handle* h, int t_lds, bool wide) {
  const int fit = gf::cov_time_matrix_sources(t_lds, wide);
  return h->tm_plan_s ? std::min(h->tm_plan_s, fit) : fit;
}

// Time matrices of every env whose graph changed since they were last built.
int ensure_time_matrix(cov_handle* h) {
  const int B = h->cfg.n_envs, Tm = h->a.Tmax;
  const int kcap = h->cfg.horizon > -1 ? h->cfg.horizon + 1 : Tm + 1;
  const int sched_stride = 4 * Tm * 16 + 16;  // motion edges <= 4 per target, batches <= 16, + prefetch slack
  if (!h->tm_cost) {
    int rc;
    if ((rc = dalloc_zero(&h->tm_cost, (size_t)B * Tm * Tm)) || (rc = dalloc_zero(&h->tm_prevT, (size_t)B * Tm * Tm)) ||
        (rc = dalloc_zero(&h->needs_random, (size_t)B * h->cfg.n_robots)) || (rc = dalloc_zero(&h->tm_envsel, (size_t)B)) ||
        (rc = dalloc_zero(&h->tm_sched, (size_t)B * sched_stride)) || (rc = dalloc_zero(&h->tm_nslots, (size_t)B)) ||
        (rc = dalloc_zero(&h->tm_lev, (size_t)B * (4 * Tm + 2))) ||
        (rc = dalloc_zero(&h->tm_nlev, (size_t)B)) || (rc = dalloc_zero(&h->tm_overflow, (size_t)B)) ||
        (rc = dalloc_zero(&h->tm_cost8, (size_t)B * Tm * Tm)) || (rc = dalloc_zero(&h->tm_wide, (size_t)B)))
      return rc;
    if (Tm <= gf::kGreedyListMaxT) {  // rows padded to 16 bytes (greedy_from_list's loads)
      h->gstride = (Tm + gf::kGreedyListPad - 1) & ~(gf::kGreedyListPad - 1);
      if ((rc = dalloc_zero(&h->tm_glist, (size_t)B * Tm * h->gstride)) || (rc = dalloc_zero(&h->tm_glen, (size_t)B * Tm)))
        return rc;
    }
    h->tm_wide_host.assign(B, 0);
  }
  std::vector<int32_t> sel;
  int t_lds = 0, e_max = 0;
  for (int b = 0; b < B; ++b) {
    if (h->tm_valid[b]) continue;
    sel.push_back(b);
    t_lds = std::max(t_lds, h->ntg_host[b]);
    e_max = std::max(e_max, h->n_motion_host[b]);
  }
  if (sel.empty()) {
    h->tm_ready = true;
    return GF_OK;
  }
  if (t_lds > COV_POOL_CAP)
    return fail(GF_EINVAL, "time matrix: a map has " + std::to_string(t_lds) + " targets, more than the " +
                               std::to_string(COV_POOL_CAP) + " the expert supports");
  // sources per wave: the widest LDS tile that holds the launch's largest map
  const int s8 = tm_sources(h, t_lds, false);
  if (int rc = ensure_tm_flags(h, s8, kcap)) return rc;
  // the schedule's edges and levels: in LDS while they fit beside the columns' state
  const bool sched_global = h->tm_plan_global || gf::cov_tm_schedule_lds_bytes(t_lds, e_max, false) > 160 * 1024;
  const int scratch_stride = 4 * e_max + 2;
  if (sched_global && sel.size() * (size_t)scratch_stride > h->tm_sched_scratch_words) {
    if (h->tm_sched_scratch) GF_HIP(hipFree(h->tm_sched_scratch));
    h->tm_sched_scratch = nullptr;
    h->tm_sched_scratch_words = 0;
    if (int rc = dalloc_zero(&h->tm_sched_scratch, sel.size() * (size_t)scratch_stride)) return rc;
    h->tm_sched_scratch_words = sel.size() * (size_t)scratch_stride;
  }
  gf::CovTmArgs t{};
  t.R = h->a.R;
  t.M = h->a.M;
  t.Tmax = Tm;
  t.horizon = h->cfg.horizon;
  t.kcap = kcap;
  t.tm_s = s8;
  t.nchunk = (Tm + s8 - 1) / s8;
  t.sched_scratch = sched_global ? h->tm_sched_scratch : nullptr;
  t.scratch_stride = scratch_stride;
  t.t_lds = t_lds;
  t.envs = h->tm_envsel;
  t.ntg = h->ntg;
  t.n_motion = h->a.n_motion;
  t.senders = h->a.senders;
  t.receivers = h->a.receivers;
  t.flags = h->tm_flags;
  t.cost = h->tm_cost;
  t.cost8 = h->tm_cost8;
  t.prevT = h->tm_prevT;
  t.sched = h->tm_sched;
  t.nslots = h->tm_nslots;
  t.nlev = h->tm_nlev;
  t.overflow = h->tm_overflow;
  t.sched_stride = sched_stride;
  t.lev_off = h->tm_lev;
  t.lev_stride = 4 * Tm + 2;  // levels <= motion edges <= 4 per target, + the end offset
  GF_HIP(hipMemcpyAsync(h->tm_envsel, sel.data(), sel.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  hipError_t e = gf::launch_cov_tm_schedule(t, (int)sel.size(), e_max, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_tm_schedule_kernel: ") + hipGetErrorString(e));
  // uint8 entries first (twice the waves per CU); envs it cannot bound get uint16
  e = gf::launch_cov_time_matrix(t, (int)sel.size(), false, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_time_matrix_kernel: ") + hipGetErrorString(e));
  std::vector<uint8_t> ovf(B);
  GF_HIP(hipMemcpyAsync(ovf.data(), h->tm_overflow, B, hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  std::vector<int32_t> wide;
  int t_wide = 0;
  for (int b : sel)
    if (ovf[b]) {
      wide.push_back(b);
      t_wide = std::max(t_wide, h->ntg_host[b]);
    }
  if (!wide.empty()) {
    const int s16 = tm_sources(h, t_wide, true);
    if (int rc = ensure_tm_flags(h, s16, kcap)) return rc;
    t.flags = h->tm_flags;
    t.tm_s = s16;
    t.nchunk = (Tm + s16 - 1) / s16;
    GF_HIP(hipMemsetAsync(h->tm_overflow, 0, B, h->stream));
    GF_HIP(hipMemcpyAsync(h->tm_envsel, wide.data(), wide.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    t.t_lds = t_wide;
    e = gf::launch_cov_time_matrix(t, (int)wide.size(), true, h->stream);
    if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_time_matrix_kernel: ") + hipGetErrorString(e));
    GF_HIP(hipStreamSynchronize(h->stream));
  }
  h->tm_wide_envs += (int64_t)wide.size();
  for (int b : sel) h->tm_wide_host[b] = 0;
  for (int b : wide) h->tm_wide_host[b] = 1;
  GF_HIP(hipMemcpyAsync(h->tm_wide, h->tm_wide_host.data(), B, hipMemcpyHostToDevice, h->stream));
  if (h->tm_glist) {  // every selected env's greedy lists, from its final matrix
    t.wide = h->tm_wide;
    t.nbr = h->a.nbr;
    t.cnt = h->a.cnt;
    t.glist = h->tm_glist;
    t.glen = h->tm_glen;
    t.gstride = h->gstride;
    GF_HIP(hipMemcpyAsync(h->tm_envsel, sel.data(), sel.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    e = gf::launch_cov_greedy_lists(t, (int)sel.size(), h->stream);
    if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_greedy_list_kernel: ") + hipGetErrorString(e));
  }
  GF_HIP(hipStreamSynchronize(h->stream));
  for (int b : sel) h->tm_valid[b] = 1;
  h->tm_ready = true;
  return GF_OK;
}

// 4 * DELTA (coverage.py:335): the module constant, whatever the env's res
constexpr double kHiddenRadius = 4.0 * 5.5;
constexpr const char* kHiddenFused =
    "a handle with hidden nodes has no fused expert (the step kernel reads the visited flags, not the expert's "
    "visited-or-undiscovered mask): take the actions from cov_controller_greedy, then cov_step";

gf::CovHiddenArgs hidden_args(const cov_handle* h) {
  gf::CovHiddenArgs g{};
  const gf::CovArgs& a = h->a;
  g.B = h->cfg.n_envs;
  g.R = a.R;
  g.M = a.M;
  g.Tmax = a.Tmax;
  g.radius = kHiddenRadius;
  g.ntg = h->ntg;
  g.tgt = h->tgt;
  g.xr = a.xr;
  g.visited = a.visited;
  g.nodes = a.nodes;
  g.senders = a.senders;
  g.receivers = a.receivers;
  g.n_motion = a.n_motion;
  g.discovered = h->discovered;
  g.hnodes = h->hnodes;
  g.hsenders = h->hsenders;
  g.gmask = h->gmask;
  g.ngmask = h->ngmask;
  g.nkeep = h->hnkeep;
  return g;
}

// Hidden handles: discovered := robots only for the n envs listed on the device (nullptr:
// every env), on the handle's stream.
int hidden_reset(cov_handle* h, const int32_t* envs, int n) {
  if (!h->hidden) return GF_OK;
  hipError_t e = gf::launch_cov_hidden_reset(hidden_args(h), envs, n, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_hidden_reset_kernel: ") + hipGetErrorString(e));
  return GF_OK;
}

// Hidden handles: the hidden observation of every env from the ordinary one, on the
// handle's stream (which the caller has ordered behind the pass that made it).
int hidden_pass(cov_handle* h) {
  if (!h->hidden) return GF_OK;
  hipError_t e = gf::launch_cov_hidden(hidden_args(h), h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_hidden_kernel: ") + hipGetErrorString(e));
  return GF_OK;
}

// Device scratch of at least `bytes` (grown on demand, reused across calls).
int scratch(cov_handle* h, size_t bytes, unsigned char** out) {
  if (bytes > h->scratch_bytes) {
    if (h->scratch) GF_HIP(hipFree(h->scratch));
    h->scratch = nullptr;
    h->scratch_bytes = 0;
    if (hipMalloc(reinterpret_cast<void**>(&h->scratch), bytes) != hipSuccess)
      return fail(GF_ENOMEM, "hipMalloc of wire-format scratch failed");
    h->scratch_bytes = bytes;
  }
  *out = h->scratch;
  return GF_OK;
}

// Edge counts of the unpack_obs tuple and their exclusive offsets.
// keep: a hidden handle's kept slots per env (hnkeep), which replace the motion + action
// edge count.
void graph_sizes(const cov_handle* h, bool mask_all, const int32_t* keep, std::vector<int32_t>& ne,
                 std::vector<int64_t>& off) {
  const int B = h->cfg.n_envs, R = h->cfg.n_robots, M = h->cfg.max_nodes;
  ne.assign(B, 0);
  off.assign(B + 1, 0);
  for (int b = 0; b < B; ++b) {
    ne[b] = (mask_all || b == 0) ? (keep ? keep[b] : h->n_motion_host[b] + 8 * R) : 4 * M;
    off[b + 1] = off[b] + ne[b];
  }
}

// A hidden handle's kept slots per env, read from the device (synchronises); empty otherwise.
int hidden_keep(cov_handle* h, std::vector<int32_t>& keep) {
  keep.clear();
  if (!h->hidden) return GF_OK;
  if (!h->has_state) return fail(GF_ESTATE, "hidden nodes: reset first (the edge counts follow the observation)");
  if (int rc = use(h)) return rc;
  keep.resize(h->cfg.n_envs);
  GF_HIP(hipMemcpyAsync(keep.data(), h->hnkeep, keep.size() * 4, hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  return GF_OK;
}

// Python's float floor division (numpy floor_divide on float64), for generate_lattice's
// `//` (make_map.py:40, :45-46).
double py_floordiv(double a, double b) {
  double mod = std::fmod(a, b);
  double div = (a - mod) / b;
  if (mod != 0.0 && ((b < 0) != (mod < 0))) div -= 1.0;
  if (div == 0.0) return std::copysign(0.0, a / b);
  double fl = std::floor(div);
  if (div - fl > 0.5) fl += 1.0;
  return fl;
}

int check_map_config(const cov_map_config* mc) {
  if (!mc) return fail(GF_EINVAL, "null map configuration");
  if (!(mc->x_max > mc->x_min) || !(mc->y_max > mc->y_min)) return fail(GF_EINVAL, "map: empty arena");
  if (!(mc->lattice_spacing > 0) || !(mc->world_radius > 0) || !(mc->road_radius > 0) || !(mc->near_radius > 0) ||
      !(mc->link_radius > 0))
    return fail(GF_EINVAL, "map: spacing and radii must be positive");
  if (mc->n_cities < 3 || mc->n_cities > gf::kMapMaxCities) return fail(GF_EINVAL, "map: n_cities must be in [3, 32]");
  return GF_OK;
}

// generate_lattice (make_map.py:30-67) with the square lattice vectors (-s, 0), (0, -s)
// (coverage.py:125-128): the points in its order as [y, x], and each point's cell
// i * NJ + j in the (arange(-nx, nx), arange(-ny, nx)) grid it sheared.
void build_lattice(const cov_map_config* mc, std::vector<double>& xy, std::vector<int32_t>& cell, int* NI, int* NJ) {
  const double s = mc->lattice_spacing;
  const double w = mc->x_max - mc->x_min, hgt = mc->y_max - mc->y_min;
  const double cx = py_floordiv(w, 2.0), cy = py_floordiv(hgt, 2.0);
  const double nx = py_floordiv(w, s), ny = py_floordiv(hgt, s);
  const int ni = static_cast<int>(std::ceil(nx - -nx)), nj = static_cast<int>(std::ceil(nx - -ny));  // np.arange lengths
  xy.clear();
  cell.clear();
  for (int i = 0; i < ni; ++i) {
    const double xs = -nx + i;
    for (int j = 0; j < nj; ++j) {
      const double ys = -ny + j;
      const double xl = -s * xs + 0.0 * ys, yl = 0.0 * xs + -s * ys;
      if (xl < w / 2.0 && xl > -w / 2.0 && yl < hgt / 2.0 && yl > -hgt / 2.0) {
        xy.push_back(yl + (cy + mc->y_min));
        xy.push_back(xl + (cx + mc->x_min));
        cell.push_back(i * nj + j);
      }
    }
  }
  *NI = ni;
  *NJ = nj;
}

// The lattice of mc on the device (rebuilt when the arena or spacing changes).
int ensure_lattice(cov_handle* h, const cov_map_config* mc) {
  const double key[5] = {mc->x_min, mc->x_max, mc->y_min, mc->y_max, mc->lattice_spacing};
  if (h->lat && std::memcmp(key, h->lat_key, sizeof(key)) == 0) return GF_OK;
  std::vector<double> xy;
  std::vector<int32_t> cell;
  int NI = 0, NJ = 0;
  build_lattice(mc, xy, cell, &NI, &NJ);
  const int L = static_cast<int>(cell.size());
  if (L < 1) return fail(GF_EINVAL, "map: the lattice has no point in the arena");
  if ((size_t)NI * NJ > (size_t)1 << 26) return fail(GF_EINVAL, "map: lattice grid too large");
  for (void* p : {static_cast<void*>(h->lat), static_cast<void*>(h->lat_cell), static_cast<void*>(h->lat_grid)})
    if (p) GF_HIP(hipFree(p));
  h->lat = nullptr;
  h->lat_cell = h->lat_grid = nullptr;
  std::vector<int32_t> grid((size_t)NI * NJ, -1);
  for (int l = 0; l < L; ++l) grid[cell[l]] = l;
  int rc;
  if ((rc = dalloc_zero(&h->lat, (size_t)L)) || (rc = dalloc_zero(&h->lat_cell, (size_t)L)) ||
      (rc = dalloc_zero(&h->lat_grid, (size_t)NI * NJ)))
    return rc;
  GF_HIP(hipMemcpy(h->lat, xy.data(), (size_t)L * 16, hipMemcpyHostToDevice));
  GF_HIP(hipMemcpy(h->lat_cell, cell.data(), (size_t)L * 4, hipMemcpyHostToDevice));
  GF_HIP(hipMemcpy(h->lat_grid, grid.data(), grid.size() * 4, hipMemcpyHostToDevice));
  h->lat_L = L;
  h->lat_NI = NI;
  h->lat_NJ = NJ;
  std::memcpy(h->lat_key, key, sizeof(key));
  return GF_OK;
}

// The envs' map streams and the map kernels' per-env outputs (allocated on first use).
int ensure_map_buffers(cov_handle* h) {
  if (h->map_cities) return GF_OK;
  const size_t B = h->cfg.n_envs;
  int rc;
  if ((rc = dalloc_zero(&h->map_key, B * gf::kMtN)) || (rc = dalloc_zero(&h->map_pos, B)) ||
      (rc = dalloc_zero(&h->map_cities, B * gf::kMapMaxCities * 2)) || (rc = dalloc_zero(&h->map_nraw, B)) ||
      (rc = dalloc_zero(&h->map_status, B)))
    return rc;
  return GF_OK;
}

int put(cov_handle* h, void* dst, const void* src, size_t bytes, bool dev_dst, bool dev_src) {
  if (!dst || !bytes) return GF_OK;
  const hipMemcpyKind k = dev_dst ? (dev_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice)
                                  : (dev_src ? hipMemcpyDeviceToHost : hipMemcpyHostToHost);
  GF_HIP(hipMemcpyAsync(dst, src, bytes, k, h->stream));
  return GF_OK;
}

}  // namespace

extern "C" {

int cov_create(const cov_config* cfg, cov_handle** out) {
  if (!cfg || !out) return fail(GF_EINVAL, "null argument");
  *out = nullptr;
  if (cfg->n_robots < 1 || cfg->n_envs < 1 || cfg->max_nodes <= cfg->n_robots)
    return fail(GF_EINVAL, "need n_robots >= 1, n_envs >= 1, max_nodes > n_robots");
  if (cfg->n_robots > 4096) return fail(GF_EINVAL, "n_robots > 4096 not supported");
  if (!(cfg->res > 0) || !(cfg->motion_radius > 0)) return fail(GF_EINVAL, "bad res/motion_radius");
  if (cfg->horizon < -1) return fail(GF_EINVAL, "horizon must be >= -1");
  if (int rc = gf::select_device(cfg->device)) return rc;
  cov_handle* h = new cov_handle();
  h->cfg = *cfg;
  const size_t B = cfg->n_envs, R = cfg->n_robots, M = cfg->max_nodes, Tm = M - R, E = 4 * M;
  gf::CovArgs& a = h->a;
  a.B = (int)B;
  a.R = (int)R;
  a.M = (int)M;
  a.Tmax = (int)Tm;
  a.episode_length = cfg->episode_length;
  a.res = cfg->res;
  a.motion_radius = cfg->motion_radius;
  int rc = GF_OK;
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_s2, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_main, hipEventDisableTiming) != hipSuccess ||
      hipEventCreate(&h->tw[0]) != hipSuccess || hipEventCreate(&h->tw[1]) != hipSuccess) {
    cov_release(h);
    return fail(GF_EHIP, "stream create failed");
  }
  if ((rc = dalloc_zero(&h->ntg, B)) || (rc = dalloc_zero(&h->tgt, B * Tm * 2)) || (rc = dalloc_zero(&a.nbr, B * Tm * 4)) ||
      (rc = dalloc_zero(&a.cnt, B * Tm)) || (rc = dalloc_zero(&a.n_motion, B)) || (rc = dalloc_zero(&a.xr, B * R * 2)) ||
      (rc = dalloc_zero(&a.cur, B * R)) || (rc = dalloc_zero(&a.visited, B * Tm)) || (rc = dalloc_zero(&a.nvisited, B)) ||
      (rc = dalloc_zero(&a.step_counter, B)) || (rc = dalloc_zero(&a.dirty, B)) || (rc = dalloc_zero(&h->actions, B * R)) ||
      (rc = dalloc_zero(&a.reward, B)) || (rc = dalloc_zero(&a.done, B)) || (rc = dalloc_zero(&a.nodes, B * M * 3)) ||
      (rc = dalloc_zero(&a.edges, B * E)) || (rc = dalloc_zero(&a.senders, B * E)) || (rc = dalloc_zero(&a.receivers, B * E)) ||
      (rc = dalloc_zero(&a.obs_step, B)) || (rc = dalloc_zero(&a.axy, B * Tm * 8)) || (rc = dalloc_zero(&a.nrec, B * Tm * 16)) || (rc = dalloc_zero(&h->err, 1)) || (rc = dalloc_zero(&h->start, B * R)) ||
      (rc = dalloc_zero(&h->visited0, B * Tm)) || (rc = dalloc_zero(&h->envsel, B))) {
    cov_release(h);
    return rc;
  }
  a.tgt = h->tgt;
  a.ntg = h->ntg;
  a.err = h->err;
  h->ntg_host.assign(B, 0);
  h->n_motion_host.assign(B, 0);
  h->tm_valid.assign(B, 0);
  *out = h;
  return GF_OK;
}

int cov_destroy(cov_handle* h) {
  cov_release(h);
  return GF_OK;
}

int cov_set_targets(cov_handle* h, int env, int n_targets, const double* targets) {
  if (!h || !targets) return fail(GF_EINVAL, "null argument");
  const int B = h->cfg.n_envs, Tm = h->a.Tmax;
  if (env >= B) return fail(GF_EINVAL, "env index out of range");
  if (n_targets < 1 || n_targets > Tm)
    return fail(GF_EINVAL, "n_targets must be in [1, max_nodes - n_robots] (PAD_NODES, coverage.py:540-543)");
  if (n_targets < h->cfg.n_robots) return fail(GF_EINVAL, "fewer targets than robots (reset draws distinct starts)");
  if (int rc = use(h)) return rc;
  const int b0 = env < 0 ? 0 : env, b1 = env < 0 ? B : env + 1;
  std::vector<int32_t> sel;
  for (int b = b0; b < b1; ++b) {
    GF_HIP(hipMemcpyAsync(h->tgt + (size_t)b * Tm * 2, targets, (size_t)n_targets * 2 * sizeof(double),
                          hipMemcpyHostToDevice, h->stream));
    h->ntg_host[b] = n_targets;
    sel.push_back(b);
  }
  GF_HIP(hipMemcpyAsync(h->ntg, h->ntg_host.data(), B * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  GF_HIP(hipMemcpyAsync(h->envsel, sel.data(), sel.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  hipError_t e = gf::launch_cov_graph(h->a, h->envsel, (int)sel.size(), h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_graph_kernel: ") + hipGetErrorString(e));
  if (int rc = hidden_reset(h, h->envsel, (int)sel.size())) return rc;
  if (int rc = check_err(h)) return rc;
  GF_HIP(hipMemcpy(h->n_motion_host.data(), h->a.n_motion, B * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int b = b0; b < b1; ++b) h->tm_valid[b] = 0;
  h->tm_ready = false;
  h->has_graph = true;
  for (int b = 0; b < B; ++b) h->has_graph = h->has_graph && h->ntg_host[b] > 0;
  return GF_OK;
}

int cov_map_lattice(const cov_map_config* mc, double* xy, int32_t* n) {
  if (!n) return fail(GF_EINVAL, "null count");
  if (int rc = check_map_config(mc)) return rc;
  std::vector<double> pts;
  std::vector<int32_t> cell;
  int NI = 0, NJ = 0;
  build_lattice(mc, pts, cell, &NI, &NJ);
  const int32_t cap = *n;
  *n = static_cast<int32_t>(cell.size());
  if (!xy) return GF_OK;
  if (cap < *n) return fail(GF_EINVAL, "lattice: the output holds fewer points than the lattice has");
  std::memcpy(xy, pts.data(), pts.size() * sizeof(double));
  return GF_OK;
}

}  // extern "C"

namespace {

// cov_generate_maps for the envs of `sel` (ascending; given cities and cities_out are rows
// of a contiguous range starting at sel[0]): one launch of each kernel over the selection.
// The outputs are indexed by position in sel.
int generate_maps_sel(cov_handle* h, const cov_map_config* mc, const std::vector<int32_t>& sel, uint64_t map_seed,
                      const double* cities, int flags, int32_t* n_targets_out, int32_t* status_out,
                      double* cities_out) {
  if (int rc = check_map_config(mc)) return rc;
  if (flags & ~(COV_MAP_SEED | COV_MAP_CITIES)) return fail(GF_EINVAL, "flags: COV_MAP_SEED | COV_MAP_CITIES");
  const bool given = flags & COV_MAP_CITIES;
  if (given && !cities) return fail(GF_EINVAL, "COV_MAP_CITIES needs the cities");
  const int B = h->cfg.n_envs, NC = mc->n_cities;
  const int nsel = (int)sel.size(), b0 = sel.empty() ? 0 : sel[0];
  if (!given && (flags & COV_MAP_SEED) && map_seed + (uint64_t)B > 0x100000000ull)
    return fail(GF_EINVAL, "map_seed + n_envs must fit in 32 bits (np.random.seed)");
  if (!given && !(flags & COV_MAP_SEED) && !h->map_seeded)
    return fail(GF_ESTATE, "the envs' map streams were never seeded (COV_MAP_SEED)");
  if (given)
    for (size_t q = 0, nq = (size_t)nsel * NC * 2; q < nq; ++q)
      if (!std::isfinite(cities[q])) return fail(GF_EINVAL, "map: the given cities hold a NaN or an infinity");
  if (int rc = use(h)) return rc;
  int rc;
  if ((rc = ensure_map_buffers(h))) return rc;
  if ((rc = ensure_lattice(h, mc))) return rc;
  // waypoints: the cities plus at most int(dist / road_radius) per Delaunay edge (at most
  // 3 NC - 6 of them, none longer than the cities' square's diagonal), within the LDS left
  const double diag = 2.0 * std::sqrt(2.0) * mc->world_radius;
  const double wbound = NC + (3.0 * NC - 6.0) * (std::floor(diag / mc->road_radius) + 1.0);
  // (a degenerate city set can have up to NC (NC - 1) / 2 roads and more waypoints than this
  // general-position bound: the kernel holds every road and reports such a map as OVERFLOW).
  // 145 KB dynamic: the kernel's static LDS (7.5 KB, the roads of all 496 city pairs
  // included) comes on top, within the CU's 160 KB
  const size_t lds_max = 145 * 1024, lds_lat = (size_t)h->lat_L * 12;
  if (lds_lat + 64 * 16 > lds_max) return fail(GF_EINVAL, "map: lattice too large for the LDS");
  // the waypoint grid of the near-road test: cells of side near_radius (1 + 2^-20) over the
  // cities' square and the arena, one cell of margin; without room for it (or for an odd
  // configuration), every lattice point scans every waypoint
  const double gh = mc->near_radius * (1.0 + 0x1p-20);
  const double gx0 = std::min(mc->x_min, -mc->world_radius) - gh, gy0 = std::min(mc->y_min, -mc->world_radius) - gh;
  const double gspan = std::max(std::max(mc->x_max, mc->world_radius) + gh - gx0, std::max(mc->y_max, mc->world_radius) + gh - gy0);
  int G = (gh > 0.0 && std::isfinite(gspan / gh) && gspan / gh < 256.0) ? static_cast<int>(std::ceil(gspan / gh)) : 0;
  const double wcap_scan = std::min<double>(wbound, (double)((lds_max - lds_lat) / 16));
  const double wfit_g = G > 0 ? ((double)lds_max - (double)lds_lat - 4.0 * G * G) / 20.0 : 0.0;
  if (wfit_g < wcap_scan) G = 0;  // the grid would cost waypoint capacity
  const int wcap = static_cast<int>(wcap_scan);
  GF_HIP(hipMemcpyAsync(h->envsel, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, h->stream));
  gf::CovMapArgs m{};
  m.n_sel = nsel;
  m.envs = h->envsel;
  m.R = h->a.R;
  m.Tmax = h->a.Tmax;
  m.NC = NC;
  m.lo = -mc->world_radius;
  m.range = mc->world_radius - -mc->world_radius;  // uniform(low, high): high - low
  m.road_radius = mc->road_radius;
  m.near_radius = mc->near_radius;
  m.link_radius = mc->link_radius;
  m.L = h->lat_L;
  m.lat = h->lat;
  m.lat_cell = h->lat_cell;
  m.cell = h->lat_grid;
  m.NI = h->lat_NI;
  m.NJ = h->lat_NJ;
  m.K = static_cast<int>(std::floor(mc->link_radius / mc->lattice_spacing)) + 1;
  m.wcap = wcap;
  m.G = G;
  m.gx0 = gx0;
  m.gy0 = gy0;
  m.gh = gh;
  m.cities = h->map_cities;
  m.mt_key = h->map_key;
  m.mt_pos = h->map_pos;
  m.seed0 = static_cast<uint32_t>(map_seed);
  m.seed = (flags & COV_MAP_SEED) ? 1 : 0;
  m.tgt = h->tgt;
  m.ntg = h->ntg;
  m.nraw = h->map_nraw;
  m.status = h->map_status;
  hipError_t e = hipSuccess;
  if (given) {
    GF_HIP(hipMemcpy2DAsync(h->map_cities + (size_t)b0 * gf::kMapMaxCities * 2, gf::kMapMaxCities * 16, cities,
                            (size_t)NC * 16, (size_t)NC * 16, nsel, hipMemcpyHostToDevice, h->stream));
  } else {
    e = gf::launch_cov_map_cities(m, h->stream);
    if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_map_cities_kernel: ") + hipGetErrorString(e));
    if (flags & COV_MAP_SEED) h->map_seeded = true;
    h->map_cfg = *mc;
    h->map_cfg_set = true;
  }
  e = gf::launch_cov_map(m, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_map_kernel: ") + hipGetErrorString(e));
  e = gf::launch_cov_graph(h->a, h->envsel, nsel, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_graph_kernel: ") + hipGetErrorString(e));
  if (int rc3 = hidden_reset(h, h->envsel, nsel)) return rc3;
  std::vector<int32_t> nraw(B), st(B), ntg(B);
  GF_HIP(hipMemcpyAsync(nraw.data(), h->map_nraw, B * 4, hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipMemcpyAsync(st.data(), h->map_status, B * 4, hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipMemcpyAsync(ntg.data(), h->ntg, B * 4, hipMemcpyDeviceToHost, h->stream));
  if (cities_out)
    GF_HIP(hipMemcpy2DAsync(cities_out, (size_t)NC * 16, h->map_cities + (size_t)b0 * gf::kMapMaxCities * 2,
                            gf::kMapMaxCities * 16, (size_t)NC * 16, nsel, hipMemcpyDeviceToHost, h->stream));
  if (int rc2 = check_err(h)) return rc2;  // synchronises; motion-graph errors (degree > 4, edges)
  GF_HIP(hipMemcpy(h->n_motion_host.data(), h->a.n_motion, B * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::string bad;
  for (int k = 0; k < nsel; ++k) {
    const int b = sel[k];
    h->ntg_host[b] = ntg[b];
    h->tm_valid[b] = 0;
    if (n_targets_out) n_targets_out[k] = nraw[b];
    if (status_out) status_out[k] = st[b];
    if (bad.empty() && (st[b] & (gf::kMapTooMany | gf::kMapTooFew | gf::kMapOverflow))) {
      bad = "env " + std::to_string(b) + ": ";
      if (st[b] & gf::kMapTooMany)
        bad += "the map has " + std::to_string(nraw[b]) + " targets, more than max_nodes - n_robots = " +
               std::to_string(h->a.Tmax) + " (the reference's padded observation cannot hold them)";
      else if (st[b] & gf::kMapTooFew)
        bad += "the map has " + std::to_string(nraw[b]) + " targets, fewer than the robots";
      else
        bad += "more road waypoints than the map kernel holds";
    }
  }
  h->tm_ready = false;
  h->has_graph = true;
  for (int b = 0; b < B; ++b) h->has_graph = h->has_graph && h->ntg_host[b] > 0;
  if (!bad.empty()) return fail(GF_EINVAL, "cov_generate_maps: " + bad);
  return GF_OK;
}

// env < 0: every env; else that env
std::vector<int32_t> env_range(const cov_handle* h, int env) {
  std::vector<int32_t> sel;
  const int B = h->cfg.n_envs;
  for (int b = env < 0 ? 0 : env; b < (env < 0 ? B : env + 1); ++b) sel.push_back(b);
  return sel;
}

}  // namespace

extern "C" {

int cov_generate_maps(cov_handle* h, const cov_map_config* mc, int env, uint64_t map_seed, const double* cities,
                      int flags, int32_t* n_targets_out, int32_t* status_out, double* cities_out) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (int rc = check_map_config(mc)) return rc;
  if (flags & ~(COV_MAP_SEED | COV_MAP_CITIES)) return fail(GF_EINVAL, "flags: COV_MAP_SEED | COV_MAP_CITIES");
  if ((flags & COV_MAP_CITIES) && !cities) return fail(GF_EINVAL, "COV_MAP_CITIES needs the cities");
  if (env >= h->cfg.n_envs) return fail(GF_EINVAL, "env index out of range");
  return generate_maps_sel(h, mc, env_range(h, env), map_seed, cities, flags, n_targets_out, status_out, cities_out);
}

int cov_get_targets(cov_handle* h, int env, double* targets) {
  if (!h || !targets || env < 0 || env >= h->cfg.n_envs) return fail(GF_EINVAL, "bad argument");
  if (h->ntg_host[env] < 1) return fail(GF_ESTATE, "the env has no target map");
  if (int rc = use(h)) return rc;
  GF_HIP(hipMemcpyAsync(targets, h->tgt + (size_t)env * h->a.Tmax * 2, (size_t)h->ntg_host[env] * 16,
                        hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  return GF_OK;
}

static_assert(COV_POOL_CAP == gf::kPoolCap && COV_MAP_NO_WINDOW == gf::kMapNoWindow, "gymflock.h and coverage_internal.h disagree");

int cov_load_occupancy(cov_handle* h, const cov_occupancy_config* oc, const uint8_t* grid, int n0, int n1,
                       int32_t* n_pool_out) {
  if (!h || !oc || !grid) return fail(GF_EINVAL, "null argument");
  if (n0 < 1 || n1 < 1 || (int64_t)n0 * n1 > (1 << 20)) return fail(GF_EINVAL, "occupancy: grid must be 1 to 2^20 cells");
  if (oc->downsample_rate < 1) return fail(GF_EINVAL, "occupancy: downsample_rate must be >= 1");
  if (!(oc->perimeter_delta >= 0.0) || !std::isfinite(oc->perimeter_delta))
    return fail(GF_EINVAL, "occupancy: perimeter_delta must be finite and >= 0");
  if (!std::isfinite(oc->xyz_min[0]) || !std::isfinite(oc->xyz_min[1])) return fail(GF_EINVAL, "occupancy: xyz_min must be finite");
  if (!(oc->num_subgraphs > 0.0) || !std::isfinite(oc->num_subgraphs))
    return fail(GF_EINVAL, "occupancy: num_subgraphs must be > 0");
  if (oc->min_targets < 1 || oc->max_tries < 1) return fail(GF_EINVAL, "occupancy: min_targets and max_tries must be >= 1");
  const double res = 0.5 * oc->downsample_rate;
  const double kd = std::floor(h->cfg.motion_radius / res) + 1.0;
  if (!(kd <= 16.0)) return fail(GF_EINVAL, "occupancy: motion_radius spans more than 16 cells of 0.5 * downsample_rate");
  // an upper bound of the pool before any launch: free cells with an occupied cell within
  // floor(perimeter_delta) cells on both axes (the kernel applies the Euclidean test)
  const int KP = (int)std::min<double>(std::floor(oc->perimeter_delta), (double)std::max(n0, n1));
  std::vector<int32_t> sum((size_t)(n0 + 1) * (n1 + 1), 0);  // occupied cells, summed-area table
  for (int i = 0; i < n0; ++i)
    for (int j = 0; j < n1; ++j)
      sum[(size_t)(i + 1) * (n1 + 1) + j + 1] = (grid[(size_t)i * n1 + j] ? 1 : 0) + sum[(size_t)i * (n1 + 1) + j + 1] +
                                                sum[(size_t)(i + 1) * (n1 + 1) + j] - sum[(size_t)i * (n1 + 1) + j];
  if (sum.back() == 0) return fail(GF_EINVAL, "occupancy: the grid has no occupied cell (from_occupancy's minimum is empty)");
  int64_t bound = 0;
  for (int i = 0; i < n0; ++i)
    for (int j = 0; j < n1; ++j) {
      if (grid[(size_t)i * n1 + j]) continue;
      const int i0 = std::max(i - KP, 0), i1 = std::min(i + KP + 1, n0), j0 = std::max(j - KP, 0), j1 = std::min(j + KP + 1, n1);
      const int occ = sum[(size_t)i1 * (n1 + 1) + j1] - sum[(size_t)i0 * (n1 + 1) + j1] - sum[(size_t)i1 * (n1 + 1) + j0] +
                      sum[(size_t)i0 * (n1 + 1) + j0];
      bound += occ > 0 ? 1 : 0;
    }
  if (bound > gf::kPoolCap)
    return fail(GF_EINVAL, "occupancy: the grid may give " + std::to_string(bound) + " targets, more than the pool holds (" +
                                std::to_string(gf::kPoolCap) + ")");
  if (int rc = use(h)) return rc;
  int rc;
  if (!h->pool_xy) {
    if ((rc = dalloc_zero(&h->pool_rawcell, (size_t)gf::kPoolCap)) || (rc = dalloc_zero(&h->pool_raw, (size_t)gf::kPoolCap)) ||
        (rc = dalloc_zero(&h->pool_cell, (size_t)gf::kPoolCap)) || (rc = dalloc_zero(&h->pool_info, (size_t)6)) ||
        (rc = dalloc_zero(&h->pool_counts, (size_t)3)) || (rc = dalloc_zero(&h->sub_tries, (size_t)h->cfg.n_envs)) ||
        (rc = dalloc_zero(&h->pool_xy, (size_t)gf::kPoolCap)))
      return rc;
  }
  h->pool_loaded = false;
  for (void* p : {static_cast<void*>(h->occ_grid), static_cast<void*>(h->pool_cellmap)})
    if (p) GF_HIP(hipFree(p));
  h->occ_grid = nullptr;
  h->pool_cellmap = nullptr;
  if ((rc = dalloc_zero(&h->occ_grid, (size_t)n0 * n1)) || (rc = dalloc_zero(&h->pool_cellmap, (size_t)n0 * n1))) return rc;
  GF_HIP(hipMemcpyAsync(h->occ_grid, grid, (size_t)n0 * n1, hipMemcpyHostToDevice, h->stream));
  gf::CovPoolArgs p{};
  p.n0 = n0;
  p.n1 = n1;
  p.grid = h->occ_grid;
  p.KP = KP;
  p.perimeter_delta = oc->perimeter_delta;
  p.res = res;
  p.xmin0 = oc->xyz_min[0];
  p.xmin1 = oc->xyz_min[1];
  p.check_connected = oc->check_connected ? 1 : 0;
  p.link_radius = h->cfg.motion_radius;
  p.K = (int)kd;
  p.num_subgraphs = oc->num_subgraphs;
  p.cell = h->pool_cellmap;
  p.raw_cell = h->pool_rawcell;
  p.raw = h->pool_raw;
  p.pool = h->pool_xy;
  p.pool_cell = h->pool_cell;
  p.info = h->pool_info;
  p.counts = h->pool_counts;
  hipError_t e = gf::launch_cov_pool(p, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_pool_kernel: ") + hipGetErrorString(e));
  int32_t counts[3] = {0, 0, 0};
  GF_HIP(hipMemcpyAsync(counts, h->pool_counts, sizeof(counts), hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipMemcpyAsync(h->pool_info_host, h->pool_info, sizeof(h->pool_info_host), hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  if (counts[2] || counts[1] > gf::kPoolCap) return fail(GF_EINVAL, "occupancy: more targets than the pool holds");
  if (counts[1] < 1) return fail(GF_EINVAL, "occupancy: no free cell within perimeter_delta of an occupied one");
  h->pool_host.assign((size_t)counts[1] * 2, 0.0);
  GF_HIP(hipMemcpy(h->pool_host.data(), h->pool_xy, (size_t)counts[1] * 16, hipMemcpyDeviceToHost));
  h->occ = *oc;
  h->pool_n = counts[1];
  h->pool_n0 = n0;
  h->pool_n1 = n1;
  h->pool_K = (int)kd;
  h->pool_loaded = true;
  if (n_pool_out) *n_pool_out = counts[1];
  return GF_OK;
}

int cov_get_pool(cov_handle* h, double* targets, double* min_xy, double* max_xy, double* subgraph_size) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->pool_loaded) return fail(GF_ESTATE, "no target pool (cov_load_occupancy)");
  if (targets) std::memcpy(targets, h->pool_host.data(), h->pool_host.size() * sizeof(double));
  if (min_xy) std::memcpy(min_xy, h->pool_info_host, 16);
  if (max_xy) std::memcpy(max_xy, h->pool_info_host + 2, 16);
  if (subgraph_size) std::memcpy(subgraph_size, h->pool_info_host + 4, 16);
  return GF_OK;
}

}  // extern "C"

namespace {

// cov_generate_submaps for the envs of `sel` (ascending; outputs and given draws indexed by
// position in sel): one launch of the sampler over the selection.
int generate_submaps_sel(cov_handle* h, const std::vector<int32_t>& sel, uint64_t map_seed, const double* draws,
                         int n_draws, int flags, int32_t* n_targets_out, int32_t* status_out, int32_t* tries_out) {
  if (flags & ~(COV_MAP_SEED | COV_MAP_DRAWS)) return fail(GF_EINVAL, "flags: COV_MAP_SEED | COV_MAP_DRAWS");
  const bool given = flags & COV_MAP_DRAWS;
  if (given && !draws) return fail(GF_EINVAL, "COV_MAP_DRAWS needs the draws");
  if (given && n_draws < 1) return fail(GF_EINVAL, "COV_MAP_DRAWS needs n_draws >= 1");
  if (given && n_draws > (1 << 20)) return fail(GF_EINVAL, "n_draws too large");
  const int B = h->cfg.n_envs, nsel = (int)sel.size();
  if (!h->pool_loaded) return fail(GF_ESTATE, "no target pool (cov_load_occupancy)");
  if (!(h->occ.num_subgraphs > 1.0))
    return fail(GF_EINVAL, "num_subgraphs <= 1 is not sampled: the map is the whole pool (cov_set_targets)");
  if (!given && (flags & COV_MAP_SEED) && map_seed + (uint64_t)B > 0x100000000ull)
    return fail(GF_EINVAL, "map_seed + n_envs must fit in 32 bits (np.random.seed)");
  if (!given && !(flags & COV_MAP_SEED) && !h->map_seeded)
    return fail(GF_ESTATE, "the envs' map streams were never seeded (COV_MAP_SEED)");
  if (gf::cov_submap_lds_bytes(h->pool_n) > 150 * 1024) return fail(GF_EINVAL, "the pool is too large for the sampler's LDS");
  if (int rc = use(h)) return rc;
  if (int rc = ensure_map_buffers(h)) return rc;
  GF_HIP(hipMemcpyAsync(h->envsel, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, h->stream));
  const double* info = h->pool_info_host;
  gf::CovSubmapArgs m{};
  m.n_sel = nsel;
  m.envs = h->envsel;
  m.R = h->a.R;
  m.Tmax = h->a.Tmax;
  m.P = h->pool_n;
  m.pool = h->pool_xy;
  m.pool_cell = h->pool_cell;
  m.cell = h->pool_cellmap;
  m.n0 = h->pool_n0;
  m.n1 = h->pool_n1;
  m.K = h->pool_K;
  m.link_radius = h->cfg.motion_radius;
  // np.random.uniform(low=min_xy, high=max_xy - subgraph_size): low + (high - low) * u
  m.lo_x = info[0];
  m.lo_y = info[1];
  m.range_x = (info[2] - info[4]) - info[0];
  m.range_y = (info[3] - info[5]) - info[1];
  m.sub_x = info[4];
  m.sub_y = info[5];
  m.min_targets = h->occ.min_targets;
  m.max_tries = h->occ.max_tries;
  m.n_draws = given ? n_draws : 0;
  m.mt_key = h->map_key;
  m.mt_pos = h->map_pos;
  m.seed0 = static_cast<uint32_t>(map_seed);
  m.seed = (flags & COV_MAP_SEED) ? 1 : 0;
  m.tgt = h->tgt;
  m.ntg = h->ntg;
  m.nraw = h->map_nraw;
  m.status = h->map_status;
  m.tries = h->sub_tries;
  if (given) {
    unsigned char* d = nullptr;
    const size_t bytes = (size_t)nsel * n_draws * 16;
    if (int rc = scratch(h, bytes, &d)) return rc;
    GF_HIP(hipMemcpyAsync(d, draws, bytes, hipMemcpyHostToDevice, h->stream));
    m.draws = reinterpret_cast<const double*>(d);
  } else if (flags & COV_MAP_SEED) {
    h->map_seeded = true;
  }
  hipError_t e = gf::launch_cov_submap(m, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_submap_kernel: ") + hipGetErrorString(e));
  e = gf::launch_cov_graph(h->a, h->envsel, nsel, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_graph_kernel: ") + hipGetErrorString(e));
  if (int rc3 = hidden_reset(h, h->envsel, nsel)) return rc3;
  std::vector<int32_t> nraw(B), st(B), tr(B), ntg(B);
  GF_HIP(hipMemcpyAsync(nraw.data(), h->map_nraw, B * 4, hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipMemcpyAsync(st.data(), h->map_status, B * 4, hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipMemcpyAsync(tr.data(), h->sub_tries, B * 4, hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipMemcpyAsync(ntg.data(), h->ntg, B * 4, hipMemcpyDeviceToHost, h->stream));
  if (int rc2 = check_err(h)) return rc2;  // synchronises; motion-graph errors (degree > 4, edges)
  GF_HIP(hipMemcpy(h->n_motion_host.data(), h->a.n_motion, B * sizeof(int32_t), hipMemcpyDeviceToHost));
  std::string bad;
  for (int k = 0; k < nsel; ++k) {
    const int b = sel[k];
    h->ntg_host[b] = ntg[b];
    h->tm_valid[b] = 0;
    if (n_targets_out) n_targets_out[k] = nraw[b];
    if (status_out) status_out[k] = st[b];
    if (tries_out) tries_out[k] = tr[b];
    if (!bad.empty()) continue;
    if (st[b] & gf::kMapTooMany)
      bad = "env " + std::to_string(b) + ": the map has " + std::to_string(nraw[b]) +
            " targets, more than max_nodes - n_robots = " + std::to_string(h->a.Tmax);
    else if (st[b] & gf::kMapTooFew)
      bad = "env " + std::to_string(b) + ": the map has " + std::to_string(nraw[b]) + " targets, fewer than the robots";
    else if ((st[b] & gf::kMapNoWindow) && !given)
      bad = "env " + std::to_string(b) + ": no window with a component of " + std::to_string(h->occ.min_targets) +
            " targets in max_tries = " + std::to_string(h->occ.max_tries) + " tries";
  }
  h->tm_ready = false;
  h->has_graph = true;
  for (int b = 0; b < B; ++b) h->has_graph = h->has_graph && h->ntg_host[b] > 0;
  if (!bad.empty()) return fail(GF_EINVAL, "cov_generate_submaps: " + bad);
  return GF_OK;
}

}  // namespace

extern "C" {

int cov_generate_submaps(cov_handle* h, int env, uint64_t map_seed, const double* draws, int n_draws, int flags,
                         int32_t* n_targets_out, int32_t* status_out, int32_t* tries_out) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (flags & ~(COV_MAP_SEED | COV_MAP_DRAWS)) return fail(GF_EINVAL, "flags: COV_MAP_SEED | COV_MAP_DRAWS");
  if ((flags & COV_MAP_DRAWS) && !draws) return fail(GF_EINVAL, "COV_MAP_DRAWS needs the draws");
  if ((flags & COV_MAP_DRAWS) && n_draws < 1) return fail(GF_EINVAL, "COV_MAP_DRAWS needs n_draws >= 1");
  if ((flags & COV_MAP_DRAWS) && n_draws > (1 << 20)) return fail(GF_EINVAL, "n_draws too large");
  if (env >= h->cfg.n_envs) return fail(GF_EINVAL, "env index out of range");
  return generate_submaps_sel(h, env_range(h, env), map_seed, draws, n_draws, flags, n_targets_out, status_out,
                              tries_out);
}

int cov_reset(cov_handle* h, const int32_t* start, const uint8_t* visited) {
  if (!h || !start || !visited) return fail(GF_EINVAL, "null argument");
  if (!h->has_graph) return fail(GF_ESTATE, "set the target graph of every env first (cov_set_targets)");
  const size_t B = h->cfg.n_envs, R = h->cfg.n_robots, Tm = h->a.Tmax;
  for (size_t b = 0; b < B; ++b)
    for (size_t i = 0; i < R; ++i)
      if (start[b * R + i] < 0 || start[b * R + i] >= h->ntg_host[b]) return fail(GF_EINVAL, "start target out of range");
  if (int rc = use(h)) return rc;
  GF_HIP(hipMemcpyAsync(h->start, start, B * R * 4, hipMemcpyHostToDevice, h->stream));
  GF_HIP(hipMemcpyAsync(h->visited0, visited, B * Tm, hipMemcpyHostToDevice, h->stream));
  hipError_t e = gf::launch_cov_reset(h->a, h->start, h->visited0, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_reset_kernel: ") + hipGetErrorString(e));
  if (int rc = hidden_reset(h, nullptr, (int)B)) return rc;
  gf::CovArgs a = h->a;
  a.actions = nullptr;
  e = gf::launch_cov_step(a, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_step_kernel: ") + hipGetErrorString(e));
  if (int rc = hidden_pass(h)) return rc;
  GF_HIP(hipStreamSynchronize(h->stream));
  h->has_state = true;
  return GF_OK;
}

int cov_reset_seeded(cov_handle* h, uint64_t seed, double frac_active, int32_t* start_out, uint8_t* visited_out) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->has_graph) return fail(GF_ESTATE, "set the target graph of every env first (cov_set_targets)");
  const size_t B = h->cfg.n_envs, R = h->cfg.n_robots, Tm = h->a.Tmax;
  if (seed + B > 0x100000000ull) return fail(GF_EINVAL, "seed + n_envs must fit in 32 bits (RandomState seeds)");
  if (!(frac_active >= 0.0 && frac_active <= 1.0)) return fail(GF_EINVAL, "frac_active must be in [0, 1]");
  if (gf::cov_seed_reset_lds_bytes((int)Tm) > 160 * 1024)  // the draw kernel's LDS: key, permutation, draws, flags
    return fail(GF_EINVAL, "max_nodes - n_robots too large for the device reset draws (draw on the host)");
  if (int rc = use(h)) return rc;
  if (!h->mt_key) {
    int rc;
    if ((rc = dalloc_zero(&h->mt_key, B * gf::kMtN)) || (rc = dalloc_zero(&h->mt_pos, B))) return rc;
  }
  gf::CovArgs a = h->a;
  a.mt_key = h->mt_key;
  a.mt_pos = h->mt_pos;
  hipError_t e = gf::launch_cov_seed_reset(a, static_cast<uint32_t>(seed), frac_active, h->start, h->visited0, h->stream);
  if (e == hipSuccess) e = gf::launch_cov_reset(h->a, h->start, h->visited0, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_reset_seeded: ") + hipGetErrorString(e));
  if (int rc = hidden_reset(h, nullptr, (int)B)) return rc;
  a = h->a;
  a.actions = nullptr;
  e = gf::launch_cov_step(a, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_step_kernel: ") + hipGetErrorString(e));
  if (int rc = hidden_pass(h)) return rc;
  if (start_out) GF_HIP(hipMemcpyAsync(start_out, h->start, B * R * 4, hipMemcpyDeviceToHost, h->stream));
  if (visited_out) GF_HIP(hipMemcpyAsync(visited_out, h->visited0, B * Tm, hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  h->has_state = true;
  return GF_OK;
}

static_assert(COV_RESET_REGION_SHORT == gf::kResetRegionShort && COV_RESET_REGION_SMALL == gf::kResetRegionSmall,
              "gymflock.h and coverage_internal.h disagree");

int cov_reset_device(cov_handle* h, const cov_reset_config* rc, const uint8_t* env_mask, int32_t* start_out,
                     uint8_t* visited_out, uint8_t* region_out, int32_t* status_out, int32_t* n_reset_out) {
  if (!h || !rc) return fail(GF_EINVAL, "null argument");
  const size_t B = h->cfg.n_envs, R = h->cfg.n_robots, Tm = h->a.Tmax;
  if (!(rc->frac_active >= 0.0 && rc->frac_active <= 1.0)) return fail(GF_EINVAL, "frac_active must be in [0, 1]");
  if (rc->nearby < 0) return fail(GF_EINVAL, "nearby must be >= 0");
  if (rc->flags & ~(COV_RESET_SEED | COV_RESET_NEW_MAPS | COV_RESET_DONE))
    return fail(GF_EINVAL, "flags: COV_RESET_SEED | COV_RESET_NEW_MAPS | COV_RESET_DONE");
  if (R > (size_t)gf::kMtN) return fail(GF_EINVAL, "device np_random draws need n_robots <= 624");
  if (gf::cov_reset_draw_lds_bytes((int)Tm) > 160 * 1024)  // key, permutation, draws, two bit sets, flags
    return fail(GF_EINVAL, "max_nodes - n_robots too large for the device reset draws (draw on the host)");
  const bool seeded = rc->flags & COV_RESET_SEED, new_maps = rc->flags & COV_RESET_NEW_MAPS;
  if (seeded && rc->seed + B > 0x100000000ull)
    return fail(GF_EINVAL, "seed + n_envs must fit in 32 bits (RandomState seeds)");
  if (n_reset_out) *n_reset_out = 0;
  if (!h->has_graph && !new_maps) return fail(GF_ESTATE, "set the target graph of every env first (cov_set_targets)");
  if (!seeded && !h->mt_key)
    return fail(GF_ESTATE, "no np_random streams on the device (cov_set_rng, cov_reset_seeded or COV_RESET_SEED)");
  const bool by_done = !env_mask && (rc->flags & COV_RESET_DONE);
  if (by_done && !h->has_state) return fail(GF_ESTATE, "COV_RESET_DONE: reset first (no done flags yet)");
  const bool sampled = h->pool_loaded && h->occ.num_subgraphs > 1.0;
  if (new_maps && !sampled && !h->map_cfg_set)
    return fail(GF_ESTATE, "COV_RESET_NEW_MAPS: no maps were drawn from the map streams yet (cov_generate_maps / "
                           "cov_generate_submaps)");
  if (int rc0 = use(h)) return rc0;
  std::vector<int32_t> sel;
  if (by_done) {
    std::vector<uint8_t> done(B);
    GF_HIP(hipMemcpyAsync(done.data(), h->a.done, B, hipMemcpyDeviceToHost, h->stream));
    GF_HIP(hipStreamSynchronize(h->stream));
    for (size_t b = 0; b < B; ++b)
      if (done[b]) sel.push_back((int32_t)b);
  } else {
    for (size_t b = 0; b < B; ++b)
      if (!env_mask || env_mask[b]) sel.push_back((int32_t)b);
  }
  const int nsel = (int)sel.size();
  if (nsel == 0) return GF_OK;
  if (!h->has_state && (size_t)nsel != B)
    return fail(GF_ESTATE, "the first reset must take every env (the others have no state yet)");
  if (new_maps) {  // the selected envs' next maps, from their own map streams
    const int rcm = sampled ? generate_submaps_sel(h, sel, 0, nullptr, 0, 0, nullptr, nullptr, nullptr)
                            : generate_maps_sel(h, &h->map_cfg, sel, 0, nullptr, 0, nullptr, nullptr, nullptr);
    if (rcm) return rcm;
  }
  if (!h->has_graph) return fail(GF_ESTATE, "set the target graph of every env first (cov_set_targets)");
  int rca;
  if (!h->mt_key && ((rca = dalloc_zero(&h->mt_key, B * gf::kMtN)) || (rca = dalloc_zero(&h->mt_pos, B)))) return rca;
  if (!h->rs_envs &&
      ((rca = dalloc_zero(&h->rs_envs, B)) || (rca = dalloc_zero(&h->rs_ok, B)) || (rca = dalloc_zero(&h->rs_region, B * Tm)) ||
       (rca = dalloc_zero(&h->rs_status, B)) || (rca = dalloc_zero(&h->rs_nregion, B)) ||
       (rca = dalloc_zero(&h->rs_start_c, B * R)) || (rca = dalloc_zero(&h->rs_visited_c, B * Tm)) ||
       (rca = dalloc_zero(&h->rs_region_c, B * Tm))))
    return rca;
  // a part of the envs: their rows also by position in the list, one copy per array
  const bool compact = (size_t)nsel != B;
  GF_HIP(hipMemcpyAsync(h->rs_envs, sel.data(), (size_t)nsel * 4, hipMemcpyHostToDevice, h->stream));
  gf::CovResetDrawArgs d{};
  d.n_sel = nsel;
  d.envs = h->rs_envs;
  d.envs_ok = h->rs_ok;
  d.R = (int)R;
  d.Tmax = (int)Tm;
  d.nearby = rc->nearby;
  d.seed = seeded ? 1 : 0;
  d.seed0 = static_cast<uint32_t>(rc->seed);
  d.frac = rc->frac_active;
  d.ntg = h->ntg;
  d.nbr = h->a.nbr;
  d.cnt = h->a.cnt;
  d.mt_key = h->mt_key;
  d.mt_pos = h->mt_pos;
  d.start = h->start;
  d.visited0 = h->visited0;
  d.region = h->rs_region;
  d.status = h->rs_status;
  d.nregion = h->rs_nregion;
  d.start_c = compact && start_out ? h->rs_start_c : nullptr;
  d.visited_c = compact && visited_out ? h->rs_visited_c : nullptr;
  d.region_c = compact && region_out ? h->rs_region_c : nullptr;
  hipError_t e = gf::launch_cov_reset_draw(d, h->stream);
  if (e == hipSuccess) e = gf::launch_cov_reset_list(h->a, h->start, h->visited0, h->rs_ok, nsel, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_reset_device: ") + hipGetErrorString(e));
  if (int rc1 = hidden_reset(h, h->rs_ok, nsel)) return rc1;
  gf::CovArgs a = h->a;
  a.actions = nullptr;
  e = gf::launch_cov_step_list(a, h->rs_ok, nsel, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_step_list_kernel: ") + hipGetErrorString(e));
  if (h->hidden) {
    e = gf::launch_cov_hidden_list(hidden_args(h), h->rs_ok, nsel, h->stream);
    if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_hidden_list_kernel: ") + hipGetErrorString(e));
  }
  // the selected envs' rows only (a struck env's start row reads -1, its visited row 1)
  std::vector<int32_t> st(B, 0), nreg(B, 0), start_h;
  std::vector<uint8_t> visited_h, region_h;
  GF_HIP(hipMemcpyAsync(st.data(), h->rs_status, B * 4, hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipMemcpyAsync(nreg.data(), h->rs_nregion, B * 4, hipMemcpyDeviceToHost, h->stream));
  if (!compact) {
    if (int rc2 = copy_out(h, start_out, h->start, B * R * 4)) return rc2;
    if (int rc2 = copy_out(h, visited_out, h->visited0, B * Tm)) return rc2;
    if (int rc2 = copy_out(h, region_out, h->rs_region, B * Tm)) return rc2;
  } else {
    if (start_out) start_h.resize((size_t)nsel * R);
    if (visited_out) visited_h.resize((size_t)nsel * Tm);
    if (region_out) region_h.resize((size_t)nsel * Tm);
    if (int rc2 = copy_out(h, start_out ? start_h.data() : nullptr, h->rs_start_c, (size_t)nsel * R * 4)) return rc2;
    if (int rc2 = copy_out(h, visited_out ? visited_h.data() : nullptr, h->rs_visited_c, (size_t)nsel * Tm)) return rc2;
    if (int rc2 = copy_out(h, region_out ? region_h.data() : nullptr, h->rs_region_c, (size_t)nsel * Tm)) return rc2;
  }
  GF_HIP(hipStreamSynchronize(h->stream));
  int small = -1, nsmall = 0;
  for (int k = 0; k < nsel; ++k) {
    const int32_t b = sel[k];
    if (status_out) status_out[b] = st[b];
    if (st[b] & gf::kResetRegionSmall) {
      if (small < 0) small = b;
      ++nsmall;
    }
    if (!compact) continue;
    if (start_out) std::memcpy(start_out + b * R, start_h.data() + (size_t)k * R, R * 4);
    if (visited_out) std::memcpy(visited_out + b * Tm, visited_h.data() + (size_t)k * Tm, Tm);
    if (region_out) std::memcpy(region_out + b * Tm, region_h.data() + (size_t)k * Tm, Tm);
  }
  if (n_reset_out) *n_reset_out = nsel - nsmall;
  if (nsmall == 0) h->has_state = true;
  if (nsmall)
    return fail(GF_EINVAL, "cov_reset_device: env " + std::to_string(small) + ": its start region has " +
                               std::to_string(nreg[small]) + " nodes, fewer than the " + std::to_string(R) +
                               " robots (numpy's choice raises); the env was not reset");
  return GF_OK;
}

int cov_set_actions(cov_handle* h, const int32_t* actions) {
  if (!h || !actions) return fail(GF_EINVAL, "null argument");
  if (int rc = use(h)) return rc;
  GF_HIP(hipMemcpyAsync(h->actions, actions, (size_t)h->cfg.n_envs * h->cfg.n_robots * 4, hipMemcpyHostToDevice,
                        h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  return GF_OK;
}

int cov_set_rng(cov_handle* h, const uint32_t* keys, const int32_t* pos) {
  if (!h || !keys || !pos) return fail(GF_EINVAL, "null argument");
  const size_t B = h->cfg.n_envs;
  if (h->cfg.n_robots > gf::kMtN)
    return fail(GF_EINVAL, "device np_random draws need n_robots <= 624 (one key regeneration per step)");
  for (size_t b = 0; b < B; ++b)
    if (pos[b] < 0 || pos[b] > gf::kMtN) return fail(GF_EINVAL, "stream position outside [0, 624]");
  if (int rc = use(h)) return rc;
  if (!h->mt_key) {
    int rc;
    if ((rc = dalloc_zero(&h->mt_key, B * gf::kMtN)) || (rc = dalloc_zero(&h->mt_pos, B))) return rc;
  }
  GF_HIP(hipMemcpyAsync(h->mt_key, keys, B * gf::kMtN * 4, hipMemcpyHostToDevice, h->stream));
  GF_HIP(hipMemcpyAsync(h->mt_pos, pos, B * 4, hipMemcpyHostToDevice, h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  return GF_OK;
}

int cov_get_rng(cov_handle* h, uint32_t* keys, int32_t* pos) {
  if (!h || !keys || !pos) return fail(GF_EINVAL, "null argument");
  if (!h->mt_key) return fail(GF_ESTATE, "no np_random streams on the device (cov_set_rng)");
  if (int rc = use(h)) return rc;
  const size_t B = h->cfg.n_envs;
  GF_HIP(hipMemcpyAsync(keys, h->mt_key, B * gf::kMtN * 4, hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipMemcpyAsync(pos, h->mt_pos, B * 4, hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  return GF_OK;
}

// n_steps fused greedy expert steps with the device fallback draws in one launch; equal to
// n_steps calls of cov_step(h, NULL, COV_ACTIONS_GREEDY | COV_GREEDY_RNG).
int cov_step_expert(cov_handle* h, int n_steps, double* rewards, uint8_t* done) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->has_state) return fail(GF_ESTATE, "reset first (cov_reset)");
  if (n_steps < 1) return fail(GF_EINVAL, "n_steps must be at least 1");
  if (h->hidden) return fail(GF_EINVAL, std::string("cov_step_expert: ") + kHiddenFused);
  if (!h->mt_key) return fail(GF_ESTATE, "set the envs' np_random streams first (cov_set_rng or cov_reset_seeded)");
  if (h->cfg.n_robots > gf::kMtN) return fail(GF_EINVAL, "n_robots <= 624 (one key regeneration per step)");
  if (int rc = use(h)) return rc;
  if (!h->tm_ready || !h->tm_glist)
    if (int rc = ensure_time_matrix(h)) return rc;
  if (!h->tm_glist) return fail(GF_EINVAL, "the fused expert needs max_nodes - n_robots <= 1024 (the greedy lists)");
  if (int rc = join_s2(h)) return rc;
  gf::CovArgsM m{};
  m.a = h->a;
  m.a.actions = nullptr;
  m.a.glist = h->tm_glist;
  m.a.glen = h->tm_glen;
  m.a.gstride = h->gstride;
  m.a.gcost = h->tm_cost;
  m.a.gprev = h->tm_prevT;
  m.a.gactions = h->actions;
  m.a.needs_random = h->needs_random;
  m.a.mt_key = h->mt_key;
  m.a.mt_pos = h->mt_pos;
  m.k_steps = n_steps;
  const size_t B = h->cfg.n_envs, n = (size_t)n_steps * B;
  unsigned char* buf = nullptr;
  if (rewards || done) {
    if (int rc = scratch(h, n * 9, &buf)) return rc;
    m.reward_k = reinterpret_cast<double*>(buf);
    m.done_k = buf + n * 8;
  }
  hipError_t e = gf::launch_cov_step_multi(m, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_step_multi_kernel: ") + hipGetErrorString(e));
  h->main_dirty = true;
  h->other_work = true;
  if (!buf) return GF_OK;
  if (int rc = copy_out(h, rewards, m.reward_k, n * 8)) return rc;
  if (int rc = copy_out(h, done, m.done_k, n)) return rc;
  GF_HIP(hipStreamSynchronize(h->stream));
  return check_err(h);
}

int cov_step(cov_handle* h, const int32_t* actions, int flags) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->has_state) return fail(GF_ESTATE, "reset first (cov_reset)");
  GF_HIP(hipSetDevice(h->cfg.device));
  if ((flags & COV_ACTIONS_GREEDY) && h->hidden) return fail(GF_EINVAL, std::string("COV_ACTIONS_GREEDY: ") + kHiddenFused);
  gf::CovArgs a = h->a;
  if ((flags & COV_GREEDY_RNG) && !(flags & COV_ACTIONS_GREEDY))
    return fail(GF_EINVAL, "COV_GREEDY_RNG needs COV_ACTIONS_GREEDY");
  if ((flags & COV_GREEDY_RNG) && !h->mt_key)
    return fail(GF_ESTATE, "COV_GREEDY_RNG: set the envs' np_random streams first (cov_set_rng)");
  if ((flags & COV_GREEDY_RNG) && h->cfg.n_robots > gf::kMtN)
    return fail(GF_EINVAL, "COV_GREEDY_RNG needs n_robots <= 624 (one key regeneration per step)");
  if (flags & COV_ACTIONS_GREEDY) {
    // controller(greedy=True) in the step's own launch, from the greedy lists
    if (!h->tm_ready || !h->tm_glist) {
      if (int rc = use(h)) return rc;
      if (int rc = ensure_time_matrix(h)) return rc;
    }
    if (!h->tm_glist) {  // Tmax > kGreedyListMaxT: the row-scan greedy kernel, then the step
      if (flags & COV_GREEDY_RNG)
        return fail(GF_EINVAL, "COV_GREEDY_RNG needs max_nodes - n_robots <= 1024 (the greedy lists)");
      if (int rc = cov_controller_greedy(h, nullptr, nullptr, nullptr)) return rc;
      return cov_step(h, nullptr, COV_ACTIONS_RESIDENT);
    }
    a.actions = nullptr;
    a.glist = h->tm_glist;
    a.glen = h->tm_glen;
    a.gstride = h->gstride;
    a.gcost = h->tm_cost;
    a.gprev = h->tm_prevT;
    a.gactions = h->actions;
    a.needs_random = h->needs_random;
    if (flags & COV_GREEDY_RNG) {
      a.mt_key = h->mt_key;
      a.mt_pos = h->mt_pos;
    }
  } else if (flags & COV_ACTIONS_DEVICE) {
    if (!actions) return fail(GF_EINVAL, "null action pointer");
    a.actions = actions;
  } else if (flags & COV_ACTIONS_RESIDENT) {
    a.actions = h->actions;
  } else {
    if (!actions) return fail(GF_EINVAL, "null action pointer");
    const size_t n = (size_t)h->cfg.n_envs * h->cfg.n_robots;
    for (size_t k = 0; k < n; ++k)
      if (actions[k] < 0 || actions[k] >= 4) return fail(GF_EINVAL, "action outside [0, 4) (coverage.py:189 index)");
    if (int rc = join_s2(h)) return rc;  // the previous second half may still read h->actions
    GF_HIP(hipMemcpyAsync(h->actions, actions, n * 4, hipMemcpyHostToDevice, h->stream));
    h->main_dirty = h->other_work = true;
    a.actions = h->actions;
  }
  const bool split = (h->nsplit == 2 || (h->nsplit == 0 && (flags & COV_ACTIONS_GREEDY))) && a.B >= 2 && !h->other_work;
  h->other_work = false;
  if (split) {
    if (h->main_dirty) {
      GF_HIP(hipEventRecord(h->ev_main, h->stream));
      GF_HIP(hipStreamWaitEvent(h->stream2, h->ev_main, 0));
      h->main_dirty = false;
    }
    gf::CovArgs a1 = a;
    a.B = (a.B + 1) / 2;
    a1.env0 = a.B;
    a1.B = h->a.B - a.B;
    hipError_t e = gf::launch_cov_step(a, h->stream);
    if (e == hipSuccess) e = gf::launch_cov_step(a1, h->stream2);
    if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_step_kernel: ") + hipGetErrorString(e));
    h->s2_pending = true;
    if (h->timing) h->tw_steps++;
    if (h->hidden) {  // one pass over every env on `stream`, behind both halves and ahead of the next ones
      if (int rc = join_s2(h)) return rc;
      if (int rc = hidden_pass(h)) return rc;
      h->main_dirty = true;
    }
    if (!(flags & (COV_ACTIONS_DEVICE | COV_ACTIONS_RESIDENT | COV_ACTIONS_GREEDY)))
      GF_HIP(hipStreamSynchronize(h->stream));
    return GF_OK;
  }
  if (int rc = join_s2(h)) return rc;
  h->main_dirty = true;
  if (h->timing && h->nsplit != 1) h->tw_steps++;  // the window counts every step
  const bool sample = h->timing && h->nsplit == 1 && (h->timing_count++ % h->timing_stride) == 0;
  if (sample) {
    if (h->ev_used + 2 > h->ev.size()) {
      for (int k = 0; k < 64; ++k) {
        hipEvent_t ev;
        GF_HIP(hipEventCreate(&ev));
        h->ev.push_back(ev);
      }
    }
    GF_HIP(hipEventRecord(h->ev[h->ev_used], h->stream));
  }
  hipError_t e = gf::launch_cov_step(a, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_step_kernel: ") + hipGetErrorString(e));
  if (int rc = hidden_pass(h)) return rc;  // inside the sampled window: the step a hidden handle pays for
  if (sample) {
    GF_HIP(hipEventRecord(h->ev[h->ev_used + 1], h->stream));
    h->ev_used += 2;
  }
  if (!(flags & (COV_ACTIONS_DEVICE | COV_ACTIONS_RESIDENT | COV_ACTIONS_GREEDY)))
    GF_HIP(hipStreamSynchronize(h->stream));
  return GF_OK;
}

}  // extern "C"

namespace {
// The device address of page-locked host memory, or nullptr (pageable; its failed
// lookup's error is cleared so later launch checks do not see it).
template <class T>
T* cov_mapped(T* p) {
  if (!p) return nullptr;
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return static_cast<T*>(d);
}
}  // namespace

extern "C" {

int cov_step_host(cov_handle* h, const int32_t* actions, float* nodes, float* edges, int32_t* senders,
                  int32_t* receivers, int64_t* step, double* reward, uint8_t* done, int32_t* closest,
                  int32_t* next_actions, uint8_t* needs_random, int flags) {
  if (!h || !actions) return fail(GF_EINVAL, "null argument");
  if (!h->has_state) return fail(GF_ESTATE, "reset first (cov_reset)");
  if (flags & ~COV_NEXT_GREEDY) return fail(GF_EINVAL, "flags: 0 or COV_NEXT_GREEDY");
  if (h->hidden) return fail(GF_EINVAL, std::string("cov_step_host: ") + kHiddenFused);
  const bool ng = flags & COV_NEXT_GREEDY;
  if (!ng && (next_actions || needs_random)) return fail(GF_EINVAL, "next_actions / needs_random need COV_NEXT_GREEDY");
  const size_t B = h->cfg.n_envs, R = h->cfg.n_robots, M = h->cfg.max_nodes, E = 4 * M, n = B * R;
  for (size_t k = 0; k < n; ++k)
    if (actions[k] < 0 || actions[k] >= 4) return fail(GF_EINVAL, "action outside [0, 4) (coverage.py:189 index)");
  // one launch on the handle's stream after everything outstanding on both streams
  if (int rc = use(h)) return rc;
  gf::CovArgs a = h->a;
  if (ng) {
    if (!h->tm_ready || !h->tm_glist)
      if (int rc = ensure_time_matrix(h)) return rc;
    if (!h->tm_glist)
      return fail(GF_EINVAL, "COV_NEXT_GREEDY needs max_nodes - n_robots <= 1024 (the per-node greedy lists)");
    a.next_greedy = 1;
    a.glist = h->tm_glist;
    a.glen = h->tm_glen;
    a.gstride = h->gstride;
    a.gcost = h->tm_cost;
    a.gprev = h->tm_prevT;
    a.gactions = h->actions;  // the next expert actions stay resident as well
    a.needs_random = h->needs_random;
  }
  // page-locked destinations are written by the step's own workgroups through their
  // mapped addresses; any other one gets a copy after the launch
  a.h_nodes = cov_mapped(nodes);
  a.h_edges = cov_mapped(edges);
  a.h_senders = cov_mapped(senders);
  a.h_receivers = cov_mapped(receivers);
  a.h_step = cov_mapped(step);
  a.h_reward = cov_mapped(reward);
  a.h_done = cov_mapped(done);
  a.h_closest = cov_mapped(closest);
  a.h_next = cov_mapped(next_actions);
  a.h_nrand = cov_mapped(needs_random);
  // the device error word of each env as its workgroup ends, in page-locked scratch
  if (!h->herr) {
    void* p = nullptr;
    if (hipHostMalloc(&p, std::max<size_t>(B, 16) * sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
      return fail(GF_ENOMEM, "hipHostMalloc (error words)");
    h->herr = static_cast<int32_t*>(p);
  }
  std::memset(h->herr, 0, B * sizeof(int32_t));
  a.h_err = cov_mapped(h->herr);
  // every destination page-locked and the actions inline: the launch is the call's only
  // device work, and the host waits for the kernel's own completion flag (done_flag.h)
  const bool fin = n * 4 <= (size_t)gf::kCovUInlineBytes && (!nodes || a.h_nodes) && (!edges || a.h_edges) &&
                   (!senders || a.h_senders) && (!receivers || a.h_receivers) && (!step || a.h_step) &&
                   (!reward || a.h_reward) && (!done || a.h_done) && (!closest || a.h_closest) &&
                   (!next_actions || a.h_next) && (!needs_random || a.h_nrand);
  if (fin) {
    if (!h->fin_cnt) {
      if (int rc = dalloc_zero(&h->fin_cnt, 1)) return rc;
      void* p = nullptr;
      if (hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
        return fail(GF_ENOMEM, "hipHostMalloc (completion flag)");
      h->fin_host = static_cast<int32_t*>(p);
      *h->fin_host = 0;
      h->fin_dev = cov_mapped(h->fin_host);
      if (!h->fin_dev) return fail(GF_EHIP, "completion flag: no mapped address");
    }
    a.fin.cnt = h->fin_cnt;
    a.fin.host = h->fin_dev;
    h->fin_seq = (h->fin_seq & 0x3fffffff) + 1;  // never 0 (the word's initial value), no overflow
    a.fin.seq = h->fin_seq;
  }
  hipError_t e;
  if (n * 4 <= (size_t)gf::kCovUInlineBytes) {
    e = gf::launch_cov_step_uin(a, actions, h->stream);  // actions in the kernel arguments
  } else {
    GF_HIP(hipMemcpyAsync(h->actions, actions, n * 4, hipMemcpyHostToDevice, h->stream));
    a.actions = h->actions;
    e = gf::launch_cov_step(a, h->stream);
  }
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_step_kernel: ") + hipGetErrorString(e));
  const gf::CovArgs& d = h->a;
  if (nodes && !a.h_nodes) GF_HIP(hipMemcpyAsync(nodes, d.nodes, B * M * 3 * 4, hipMemcpyDeviceToHost, h->stream));
  if (edges && !a.h_edges) GF_HIP(hipMemcpyAsync(edges, d.edges, B * E * 4, hipMemcpyDeviceToHost, h->stream));
  if (senders && !a.h_senders) GF_HIP(hipMemcpyAsync(senders, d.senders, B * E * 4, hipMemcpyDeviceToHost, h->stream));
  if (receivers && !a.h_receivers)
    GF_HIP(hipMemcpyAsync(receivers, d.receivers, B * E * 4, hipMemcpyDeviceToHost, h->stream));
  if (step && !a.h_step) GF_HIP(hipMemcpyAsync(step, d.obs_step, B * 8, hipMemcpyDeviceToHost, h->stream));
  if (reward && !a.h_reward) GF_HIP(hipMemcpyAsync(reward, d.reward, B * 8, hipMemcpyDeviceToHost, h->stream));
  if (done && !a.h_done) GF_HIP(hipMemcpyAsync(done, d.done, B, hipMemcpyDeviceToHost, h->stream));
  if (closest && !a.h_closest) GF_HIP(hipMemcpyAsync(closest, d.cur, n * 4, hipMemcpyDeviceToHost, h->stream));
  if (next_actions && !a.h_next) GF_HIP(hipMemcpyAsync(next_actions, h->actions, n * 4, hipMemcpyDeviceToHost, h->stream));
  if (needs_random && !a.h_nrand)
    GF_HIP(hipMemcpyAsync(needs_random, h->needs_random, n, hipMemcpyDeviceToHost, h->stream));
  if (fin) {
    const hipError_t q = gf::wait_done(h->fin_host, h->fin_seq, h->stream);
    if (q == hipErrorUnknown) return fail(GF_EHIP, "cov_step_host: the step finished without its completion flag");
    if (q != hipSuccess) return fail(GF_EHIP, std::string("cov_step_host: ") + hipGetErrorString(q));
  } else {
    // spin on the stream: a drop-in step is latency-bound (a blocking wait's wake-up
    // costs a sizeable part of it)
    for (;;) {
      const hipError_t q = hipStreamQuery(h->stream);
      if (q == hipSuccess) break;
      if (q != hipErrorNotReady) return fail(GF_EHIP, std::string("cov_step_host: ") + hipGetErrorString(q));
    }
  }
  int err = 0;
  for (size_t b = 0; b < B; ++b) err |= h->herr[b];
  if (err) return check_err(h);  // reads, clears and reports the device error word
  return GF_OK;
}

int cov_kernel_timing(cov_handle* h, int enable, double* avg_ms, int64_t* launches) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (int rc = use(h)) return rc;
  GF_HIP(hipStreamSynchronize(h->stream));
  if (enable >= 1) {  // start: time every enable-th step launch
    h->ev_used = 0;
    h->timing = true;
    h->timing_stride = enable;
    h->timing_count = 0;
    h->tw_steps = 0;  // split steps: one window, device time per step
    GF_HIP(hipEventRecord(h->tw[0], h->stream));
    h->other_work = false;  // both streams idle: the first timed step splits like the rest
    return GF_OK;
  }
  if (h->tw_steps > 0) {
    GF_HIP(hipEventRecord(h->tw[1], h->stream));
    GF_HIP(hipEventSynchronize(h->tw[1]));
    float ms = 0;
    GF_HIP(hipEventElapsedTime(&ms, h->tw[0], h->tw[1]));
    if (avg_ms) *avg_ms = ms / h->tw_steps;
    if (launches) *launches = h->tw_steps;
    if (enable == 0) h->timing = false;
    else {
      h->tw_steps = 0;
      GF_HIP(hipEventRecord(h->tw[0], h->stream));
    }
    return GF_OK;
  }
  double tot = 0;
  for (size_t k = 0; k + 1 < h->ev_used; k += 2) {
    float ms = 0;
    GF_HIP(hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1]));
    tot += ms;
  }
  const int64_t n = (int64_t)(h->ev_used / 2);
  if (avg_ms) *avg_ms = n ? tot / n : 0.0;
  if (launches) *launches = n;
  if (enable == 0) h->timing = false;
  return GF_OK;
}

int cov_set_robot_positions(cov_handle* h, int env, const double* xr) {
  if (!h || !xr || env < 0 || env >= h->cfg.n_envs) return fail(GF_EINVAL, "bad argument");
  if (!h->has_state) return fail(GF_ESTATE, "reset first (cov_reset)");
  if (int rc = use(h)) return rc;
  const size_t R = h->cfg.n_robots;
  const uint8_t one = 1;
  GF_HIP(hipMemcpyAsync(h->a.xr + env * R * 2, xr, R * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  GF_HIP(hipMemcpyAsync(h->a.dirty + env, &one, 1, hipMemcpyHostToDevice, h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  return GF_OK;
}

int cov_get_obs(cov_handle* h, int env, float* nodes, float* edges, int32_t* senders, int32_t* receivers,
                int64_t* step) {
  if (!h || env < 0 || env >= h->cfg.n_envs) return fail(GF_EINVAL, "bad argument");
  // before the first reset the arrays hold the graph's static part (the motion edges the
  // env's nearby-starts draw walks, coverage.py:655-673); the robots' part follows reset
  if (!h->has_state && !h->has_graph) return fail(GF_ESTATE, "set the targets (cov_set_targets) or reset first");
  if (int rc = use(h)) return rc;
  const size_t M = h->cfg.max_nodes, E = 4 * M;
  const gf::CovArgs& a = h->a;
  if (int rc = copy_out(h, nodes, a.nodes + env * M * 3, M * 3 * 4)) return rc;
  if (int rc = copy_out(h, edges, a.edges + env * E, E * 4)) return rc;
  if (int rc = copy_out(h, senders, a.senders + env * E, E * 4)) return rc;
  if (int rc = copy_out(h, receivers, a.receivers + env * E, E * 4)) return rc;
  if (int rc = copy_out(h, step, a.obs_step + env, 8)) return rc;
  GF_HIP(hipStreamSynchronize(h->stream));
  return check_err(h);
}

int cov_get_rewards(cov_handle* h, double* reward, uint8_t* done) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (int rc = use(h)) return rc;
  const size_t B = h->cfg.n_envs;
  if (int rc = copy_out(h, reward, h->a.reward, B * 8)) return rc;
  if (int rc = copy_out(h, done, h->a.done, B)) return rc;
  GF_HIP(hipStreamSynchronize(h->stream));
  return check_err(h);
}

int cov_get_robots(cov_handle* h, int env, double* xr, int32_t* nodes) {
  if (!h || env < 0 || env >= h->cfg.n_envs) return fail(GF_EINVAL, "bad argument");
  if (int rc = use(h)) return rc;
  const size_t R = h->cfg.n_robots;
  if (int rc = copy_out(h, xr, h->a.xr + env * R * 2, R * 16)) return rc;
  if (int rc = copy_out(h, nodes, h->a.cur + env * R, R * 4)) return rc;
  GF_HIP(hipStreamSynchronize(h->stream));
  return GF_OK;
}

int cov_get_visited(cov_handle* h, int env, uint8_t* visited) {
  if (!h || !visited || env < 0 || env >= h->cfg.n_envs) return fail(GF_EINVAL, "bad argument");
  if (int rc = use(h)) return rc;
  const size_t Tm = h->a.Tmax;
  if (int rc = copy_out(h, visited, h->a.visited + env * Tm, Tm)) return rc;
  GF_HIP(hipStreamSynchronize(h->stream));
  return GF_OK;
}

int cov_get_n_motion(cov_handle* h, int32_t* n_motion) {
  if (!h || !n_motion) return fail(GF_EINVAL, "null argument");
  if (int rc = use(h)) return rc;
  if (int rc = copy_out(h, n_motion, h->a.n_motion, (size_t)h->cfg.n_envs * 4)) return rc;
  GF_HIP(hipStreamSynchronize(h->stream));
  return GF_OK;
}

int cov_get_n_targets(cov_handle* h, int32_t* n_targets) {
  if (!h || !n_targets) return fail(GF_EINVAL, "null argument");
  for (int b = 0; b < h->cfg.n_envs; ++b) n_targets[b] = h->ntg_host[b];
  return GF_OK;
}

int cov_controller_greedy(cov_handle* h, int32_t* actions, uint8_t* needs_random, int64_t* n_random) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->has_state) return fail(GF_ESTATE, "reset first (cov_reset)");
  if (int rc = use(h)) return rc;
  if (int rc = ensure_time_matrix(h)) return rc;
  gf::CovGreedyArgs g{};
  const gf::CovArgs& a = h->a;
  g.B = a.B;
  g.R = a.R;
  g.Tmax = a.Tmax;
  g.ntg = h->ntg;
  g.tgt = h->tgt;
  g.xr = a.xr;
  g.dirty = a.dirty;
  g.cur = a.cur;
  g.cost = h->tm_cost;
  g.cost8 = h->tm_cost8;
  g.wide = h->tm_wide;
  g.prevT = h->tm_prevT;
  // hidden nodes: controller()'s second mask (coverage.py:819-820) joins the first, and with
  // it the column-0 quirk: any_vis is true when any target is visited or undiscovered
  g.visited = h->hidden ? h->gmask : a.visited;
  g.nvisited = h->hidden ? h->ngmask : a.nvisited;
  g.nbr = a.nbr;
  g.cnt = a.cnt;
  g.actions = h->actions;
  g.needs_random = h->needs_random;
  g.err = h->err;
  g.glist = h->tm_glist;
  g.glen = h->tm_glen;
  g.gstride = h->gstride;
  hipError_t e = gf::launch_cov_greedy(g, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_greedy_kernel: ") + hipGetErrorString(e));
  if (!actions && !needs_random && !n_random) return GF_OK;
  const size_t n = (size_t)a.B * a.R;
  std::vector<uint8_t> mask;
  uint8_t* rnd = needs_random;
  if (n_random && !rnd) {
    mask.resize(n);
    rnd = mask.data();
  }
  if (int rc = copy_out(h, actions, h->actions, n * 4)) return rc;
  if (int rc = copy_out(h, rnd, h->needs_random, n)) return rc;
  GF_HIP(hipStreamSynchronize(h->stream));
  if (n_random) {
    int64_t cnt = 0;
    for (size_t k = 0; k < n; ++k) cnt += rnd[k] ? 1 : 0;
    *n_random = cnt;
  }
  return check_err(h);
}

int cov_get_actions(cov_handle* h, int32_t* actions, uint8_t* needs_random) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (int rc = use(h)) return rc;
  const size_t n = (size_t)h->cfg.n_envs * h->cfg.n_robots;
  if (int rc = copy_out(h, actions, h->actions, n * 4)) return rc;
  if (needs_random) {
    if (h->needs_random) {
      if (int rc = copy_out(h, needs_random, h->needs_random, n)) return rc;
    } else {
      std::memset(needs_random, 0, n);
    }
  }
  GF_HIP(hipStreamSynchronize(h->stream));
  return GF_OK;
}

int cov_get_time_matrix(cov_handle* h, int env, int32_t* cost, int32_t* prev) {
  if (!h || env < 0 || env >= h->cfg.n_envs) return fail(GF_EINVAL, "bad argument");
  if (!h->has_graph) return fail(GF_ESTATE, "set the target graph first (cov_set_targets)");
  if (int rc = use(h)) return rc;
  if (int rc = ensure_time_matrix(h)) return rc;
  const size_t Tm = h->a.Tmax, T = h->ntg_host[env];
  std::vector<uint16_t> c(Tm * Tm);
  std::vector<int16_t> p(Tm * Tm);
  GF_HIP(hipMemcpyAsync(c.data(), h->tm_cost + env * Tm * Tm, Tm * Tm * 2, hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipMemcpyAsync(p.data(), h->tm_prevT + env * Tm * Tm, Tm * Tm * 2, hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < T; ++i)
    for (size_t j = 0; j < T; ++j) {
      if (cost) cost[i * T + j] = c[i * Tm + j] == 0xFFFF ? 1000 : c[i * Tm + j];
      if (prev) prev[i * T + j] = p[j * Tm + i];  // graph_previous[i, j] lives at prevT[j][i]
    }
  return GF_OK;
}

int cov_get_flat_obs(cov_handle* h, void* dst, int flags) {
  if (!h || !dst) return fail(GF_EINVAL, "null argument");
  if (!h->has_state) return fail(GF_ESTATE, "reset first (cov_reset)");
  if (int rc = use(h)) return rc;
  const bool f32 = flags & COV_FLAT_F32;
  const int nf = h->hidden ? 4 : 3;
  const size_t bytes = (size_t)h->cfg.n_envs * ((size_t)(12 + nf) * h->cfg.max_nodes + 1) * (f32 ? 4 : 8);
  void* out = dst;
  if (!(flags & COV_OUT_DEVICE)) {
    unsigned char* sc = nullptr;
    if (int rc = scratch(h, bytes, &sc)) return rc;
    out = sc;
  }
  gf::CovArgs fa = h->a;
  if (h->hidden) {
    fa.nodes = h->hnodes;
    fa.senders = h->hsenders;
  }
  hipError_t e = gf::launch_cov_flat_obs(fa, nf, out, f32, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_flat_obs_kernel: ") + hipGetErrorString(e));
  if (flags & COV_OUT_DEVICE) return GF_OK;  // stream-ordered; cov_sync before reading
  GF_HIP(hipMemcpyAsync(dst, out, bytes, hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  return check_err(h);
}

int cov_graphs_tuple_sizes(cov_handle* h, int32_t* n_edge, int64_t* total_edges, int flags) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->has_graph) return fail(GF_ESTATE, "set the target graph first (cov_set_targets)");
  std::vector<int32_t> ne, keep;
  std::vector<int64_t> off;
  if (int rc = hidden_keep(h, keep)) return rc;
  graph_sizes(h, flags & COV_MASK_ALL, h->hidden ? keep.data() : nullptr, ne, off);
  if (n_edge) std::memcpy(n_edge, ne.data(), ne.size() * sizeof(int32_t));
  if (total_edges) *total_edges = off.back();
  return GF_OK;
}

int cov_get_graphs_tuple(cov_handle* h, int32_t* n_node, float* nodes, int32_t* n_edge, float* edges,
                         int32_t* senders, int32_t* receivers, float* globs, int flags) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->has_state) return fail(GF_ESTATE, "reset first (cov_reset)");
  if ((edges != nullptr) != (senders != nullptr) || (edges != nullptr) != (receivers != nullptr))
    return fail(GF_EINVAL, "edges, senders and receivers go together (all or none)");
  if (int rc = use(h)) return rc;
  const bool dev = flags & COV_OUT_DEVICE;
  const int B = h->cfg.n_envs, M = h->cfg.max_nodes;
  std::vector<int32_t> ne, keep;
  std::vector<int64_t> off;
  if (int rc = hidden_keep(h, keep)) return rc;
  graph_sizes(h, flags & COV_MASK_ALL, h->hidden ? keep.data() : nullptr, ne, off);
  const int64_t total = off.back();
  if (!h->goff)
    if (hipMalloc(reinterpret_cast<void**>(&h->goff), (B + 1) * sizeof(int64_t)) != hipSuccess)
      return fail(GF_ENOMEM, "hipMalloc of graph offsets failed");
  GF_HIP(hipMemcpyAsync(h->goff, off.data(), (B + 1) * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  if (edges) {
    float* e_out = edges;
    int32_t *s_out = senders, *r_out = receivers;
    if (!dev) {
      unsigned char* sc = nullptr;
      if (int rc = scratch(h, (size_t)total * 12, &sc)) return rc;
      e_out = reinterpret_cast<float*>(sc);
      s_out = reinterpret_cast<int32_t*>(sc + (size_t)total * 4);
      r_out = reinterpret_cast<int32_t*>(sc + (size_t)total * 8);
    }
    hipError_t e = h->hidden ? gf::launch_cov_hidden_graphs(hidden_args(h), h->a.edges, h->goff, flags & COV_MASK_ALL,
                                                            e_out, s_out, r_out, h->stream)
                             : gf::launch_cov_graphs(h->a, h->goff, flags & COV_MASK_ALL, e_out, s_out, r_out, h->stream);
    if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_graphs_kernel: ") + hipGetErrorString(e));
    if (!dev) {
      if (int rc = put(h, edges, e_out, (size_t)total * 4, false, true)) return rc;
      if (int rc = put(h, senders, s_out, (size_t)total * 4, false, true)) return rc;
      if (int rc = put(h, receivers, r_out, (size_t)total * 4, false, true)) return rc;
    }
  }
  if (int rc = put(h, nodes, h->hidden ? h->hnodes : h->a.nodes, (size_t)B * M * (h->hidden ? 4 : 3) * sizeof(float), dev, true))
    return rc;
  std::vector<int32_t> nn(B, M);
  if (int rc = put(h, n_node, nn.data(), B * sizeof(int32_t), dev, false)) return rc;
  if (int rc = put(h, n_edge, ne.data(), B * sizeof(int32_t), dev, false)) return rc;
  std::vector<float> gl(B);
  if (globs) {
    std::vector<int64_t> st(B);
    GF_HIP(hipMemcpyAsync(st.data(), h->a.obs_step, B * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    GF_HIP(hipStreamSynchronize(h->stream));
    for (int b = 0; b < B; ++b) gl[b] = static_cast<float>(st[b]);
    if (int rc = put(h, globs, gl.data(), B * sizeof(float), dev, false)) return rc;
  }
  GF_HIP(hipStreamSynchronize(h->stream));  // host temporaries above
  return check_err(h);
}

int cov_set_streams(cov_handle* h, int n) {
  if (!h || n < 0 || n > 2) return fail(GF_EINVAL, "n must be 0 (auto), 1 or 2");
  if (int rc = use(h)) return rc;
  h->nsplit = n;
  return GF_OK;
}

int cov_set_tm_plan(cov_handle* h, int sources_per_wave, int schedule_in_global) {
  if (!h) return fail(GF_EINVAL, "null handle");
  const int S = sources_per_wave;
  if (S != 0 && S != 8 && S != 16 && S != 32 && S != 64) return fail(GF_EINVAL, "sources_per_wave must be 0 (auto), 8, 16, 32 or 64");
  if (schedule_in_global != 0 && schedule_in_global != 1) return fail(GF_EINVAL, "schedule_in_global must be 0 or 1");
  // the uint8 tile of the largest map the handle can hold (the uint16 rerun narrows it where it must)
  if (S && gf::cov_time_matrix_lds_bytes(h->a.Tmax, false, S) > 160 * 1024)
    return fail(GF_EINVAL, "sources_per_wave: (max_nodes - n_robots + 1) * " + std::to_string(S) +
                               " bytes exceed the 160 KB LDS of a CU");
  if (int rc = use(h)) return rc;
  h->tm_plan_s = S;
  h->tm_plan_global = schedule_in_global;
  std::fill(h->tm_valid.begin(), h->tm_valid.end(), 0);
  h->tm_ready = false;
  return GF_OK;
}

int cov_set_hidden(cov_handle* h, int enable) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (enable != 0 && enable != 1) return fail(GF_EINVAL, "enable must be 0 or 1");
  if (int rc = use(h)) return rc;
  if (!enable) {
    h->hidden = false;
    return GF_OK;
  }
  const size_t B = h->cfg.n_envs, M = h->cfg.max_nodes, Tm = h->a.Tmax;
  if (gf::cov_hidden_lds_bytes(h->cfg.n_robots, h->cfg.max_nodes) > 64 * 1024)
    return fail(GF_EINVAL, "hidden nodes: n_robots * 16 + max_nodes / 4 bytes exceed the pass's 64 KB of LDS");
  if (!h->discovered) {
    int rc;
    if ((rc = dalloc_zero(&h->discovered, B * M)) || (rc = dalloc_zero(&h->hnodes, B * M * 4)) ||
        (rc = dalloc_zero(&h->hsenders, B * 4 * M)) || (rc = dalloc_zero(&h->gmask, B * Tm)) ||
        (rc = dalloc_zero(&h->ngmask, B)) || (rc = dalloc_zero(&h->hnkeep, B)))
      return rc;
  }
  h->hidden = true;
  if (int rc = hidden_reset(h, nullptr, (int)B)) return rc;
  // an observation taken before this call gets its hidden form at once
  if (h->has_state)
    if (int rc = hidden_pass(h)) return rc;
  GF_HIP(hipStreamSynchronize(h->stream));
  return GF_OK;
}

int cov_get_hidden_obs(cov_handle* h, int env, float* nodes4, int32_t* senders, uint8_t* discovered) {
  if (!h || env < 0 || env >= h->cfg.n_envs) return fail(GF_EINVAL, "bad argument");
  if (!h->hidden) return fail(GF_ESTATE, "the handle does not hide nodes (cov_set_hidden)");
  if ((nodes4 || senders) && !h->has_state) return fail(GF_ESTATE, "reset first (cov_reset)");
  if (int rc = use(h)) return rc;
  const size_t M = h->cfg.max_nodes;
  if (int rc = copy_out(h, nodes4, h->hnodes + env * M * 4, M * 4 * 4)) return rc;
  if (int rc = copy_out(h, senders, h->hsenders + env * M * 4, M * 4 * 4)) return rc;
  if (int rc = copy_out(h, discovered, h->discovered + env * M, M)) return rc;
  GF_HIP(hipStreamSynchronize(h->stream));
  return check_err(h);
}

int64_t cov_explore_lds_bytes(int n_robots, int max_nodes) {
  if (n_robots < 1 || max_nodes < n_robots) return -1;
  return (int64_t)gf::cov_explore_lds_layout(n_robots, max_nodes, nullptr, nullptr);
}

// n_steps expert steps of a handle that hides nodes in one launch (cov_explore_multi_kernel);
// equal to n_steps times cov_controller_greedy, the host's fallback draws, cov_set_actions and
// the resident cov_step with its hidden pass.
int cov_explore_expert(cov_handle* h, int n_steps, const cov_rollout* rec) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->hidden) return fail(GF_ESTATE, "cov_explore_expert: the handle does not hide nodes (cov_set_hidden); cov_step_expert is its form");
  if (!h->has_state) return fail(GF_ESTATE, "reset first (cov_reset)");
  if (!h->mt_key) return fail(GF_ESTATE, "set the envs' np_random streams first (cov_set_rng or cov_reset_seeded)");
  if (n_steps < 1) return fail(GF_EINVAL, "n_steps must be at least 1");
  const int every = rec ? rec->record_every : 1;
  if (every < 1 || n_steps % every != 0) return fail(GF_EINVAL, "record_every must be at least 1 and divide n_steps");
  if (rec && (rec->flags & ~COV_ROLLOUT_DEVICE)) return fail(GF_EINVAL, "unknown cov_rollout flags");
  const int R = h->cfg.n_robots, M = h->cfg.max_nodes;
  if (R > gf::kMtN) return fail(GF_EINVAL, "n_robots <= 624 (one key regeneration per step)");
  const size_t lds = gf::cov_explore_lds_layout(R, M, nullptr, nullptr);
  if (lds > gf::kCovExploreLdsMax)
    return fail(GF_EINVAL, "cov_explore_expert: " + std::to_string(lds) + " bytes of LDS per workgroup exceed 64 KB (cov_explore_lds_bytes)");
  if (M - R > gf::kGreedyListMaxT)
    return fail(GF_EINVAL, "the fused expert needs max_nodes - n_robots <= 1024 (the greedy lists)");
  if (int rc = use(h)) return rc;
  if (!h->tm_ready || !h->tm_glist)
    if (int rc = ensure_time_matrix(h)) return rc;
  if (!h->tm_glist) return fail(GF_EINVAL, "the fused expert needs max_nodes - n_robots <= 1024 (the greedy lists)");
  if (int rc = join_s2(h)) return rc;
  gf::CovArgsX x{};
  x.a = h->a;
  x.a.actions = nullptr;
  x.a.glist = h->tm_glist;
  x.a.glen = h->tm_glen;
  x.a.gstride = h->gstride;
  x.a.gcost = h->tm_cost;
  x.a.gprev = h->tm_prevT;
  x.a.gactions = h->actions;
  x.a.needs_random = h->needs_random;
  x.a.mt_key = h->mt_key;
  x.a.mt_pos = h->mt_pos;
  x.h = hidden_args(h);
  x.n_steps = n_steps;
  x.record_every = every;
  const size_t B = h->cfg.n_envs, n = (size_t)n_steps * B, K = (size_t)(n_steps / every);
  const size_t L = (size_t)16 * M + 1;
  const bool dev = rec && (rec->flags & COV_ROLLOUT_DEVICE);
  // host destinations: one scratch block, each record 16-byte aligned
  size_t off[5] = {0, 0, 0, 0, 0}, bytes[5] = {0, 0, 0, 0, 0};
  unsigned char* buf = nullptr;
  if (rec && dev) {
    x.reward_k = rec->rewards;
    x.done_k = rec->done;
    x.act_k = rec->actions;
    x.nrand_k = rec->needs_random;
    x.flat_k = rec->flat_obs;
  } else if (rec) {
    const void* dst[5] = {rec->rewards, rec->done, rec->actions, rec->needs_random, rec->flat_obs};
    const size_t want[5] = {n * 8, n, n * R * 4, n * R, K * B * L * 4};
    size_t total = 0;
    for (int k = 0; k < 5; ++k) {
      off[k] = total;
      bytes[k] = dst[k] ? want[k] : 0;
      total += (bytes[k] + 15) & ~(size_t)15;
    }
    if (total) {
      if (int rc = scratch(h, total, &buf)) return rc;
      if (bytes[0]) x.reward_k = reinterpret_cast<double*>(buf + off[0]);
      if (bytes[1]) x.done_k = buf + off[1];
      if (bytes[2]) x.act_k = reinterpret_cast<int32_t*>(buf + off[2]);
      if (bytes[3]) x.nrand_k = buf + off[3];
      if (bytes[4]) x.flat_k = reinterpret_cast<float*>(buf + off[4]);
    }
  }
  hipError_t e = gf::launch_cov_explore_multi(x, h->stream);
  if (e != hipSuccess) return fail(GF_EHIP, std::string("cov_explore_multi_kernel: ") + hipGetErrorString(e));
  h->main_dirty = true;
  h->other_work = true;
  if (!buf) return GF_OK;
  void* dst[5] = {rec->rewards, rec->done, rec->actions, rec->needs_random, rec->flat_obs};
  for (int k = 0; k < 5; ++k)
    if (bytes[k])
      if (int rc = copy_out(h, dst[k], buf + off[k], bytes[k])) return rc;
  GF_HIP(hipStreamSynchronize(h->stream));
  return check_err(h);
}

int cov_sync(cov_handle* h) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (int rc = use(h)) return rc;
  GF_HIP(hipStreamSynchronize(h->stream));
  // both streams idle: the next step may split. main_dirty stays set (use_dev): reads of
  // the outputs a zero-copy consumer enqueues on `stream` after this call come before
  // the next step's second half
  h->other_work = false;
  return check_err(h);
}

}  // extern "C"
