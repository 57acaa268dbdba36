// C-ABI of the Coverage-v0 engine, what moves the envs (include/gymflock.h): the time
// matrices and greedy lists, the three resets, cov_step, cov_step_host, the three expert
// rollouts and cov_controller_greedy.
#include <algorithm>
#include <cstring>

#include "cov_handle.h"

using namespace gf;  // capi_common.h's helpers and cov_handle.h's internal calls

namespace {

// The time-matrix flags (B, nchunk, kcap) for tiles of S sources per wave.
int ensure_tm_flags(cov_handle* h, int S, int kcap) {
  const size_t need = (size_t)h->cfg.n_envs * ((h->a.Tmax + S - 1) / S) * kcap;
  return h->mem.grow_zeroed(&h->tm_flags, &h->tm_flags_bytes, need);
}

// Sources per wave for a time-matrix pass over maps of up to t_lds targets: the plan's
// (cov_set_tm_plan, narrowed where this launch's maps need it) or the largest whose tile fits.
int tm_sources(const cov_handle* h, int t_lds, bool wide) {
  const int fit = gf::cov_time_matrix_sources(t_lds, wide);
  return h->tm_plan_s ? std::min(h->tm_plan_s, fit) : fit;
}

// The greedy lists, for each kernel argument struct that carries them.
template <class Args>
void greedy_lists(const cov_handle* h, Args& a) {
  a.glist = h->tm_glist;
  a.glen = h->tm_glen;
  a.gstride = h->gstride;
}

}  // namespace

int gf::ensure_time_matrix(cov_handle* h) {
  const int B = h->cfg.n_envs, Tm = h->a.Tmax;
  const int kcap = h->cfg.horizon > -1 ? h->cfg.horizon + 1 : Tm + 1;
  const int sched_stride = 4 * Tm * 16 + 16;  // motion edges <= 4 per target, batches <= 16, + prefetch slack
  gf::DeviceBuffers& m = h->mem;
  if (!h->tm_cost) {
    int rc;
    if ((rc = m.zeroed(&h->tm_cost, (size_t)B * Tm * Tm)) || (rc = m.zeroed(&h->tm_prevT, (size_t)B * Tm * Tm)) ||
        (rc = m.zeroed(&h->needs_random, (size_t)B * h->cfg.n_robots)) || (rc = m.zeroed(&h->tm_envsel, (size_t)B)) ||
        (rc = m.zeroed(&h->tm_sched, (size_t)B * sched_stride)) || (rc = m.zeroed(&h->tm_nslots, (size_t)B)) ||
        (rc = m.zeroed(&h->tm_lev, (size_t)B * (4 * Tm + 2))) ||
        (rc = m.zeroed(&h->tm_nlev, (size_t)B)) || (rc = m.zeroed(&h->tm_overflow, (size_t)B)) ||
        (rc = m.zeroed(&h->tm_cost8, (size_t)B * Tm * Tm)) || (rc = m.zeroed(&h->tm_wide, (size_t)B)))
      return rc;
    if (Tm <= gf::kGreedyListMaxT) {  // rows padded to 16 bytes (greedy_from_list's loads)
      h->gstride = (Tm + gf::kGreedyListPad - 1) & ~(gf::kGreedyListPad - 1);
      if ((rc = m.zeroed(&h->tm_glist, (size_t)B * Tm * h->gstride)) || (rc = m.zeroed(&h->tm_glen, (size_t)B * Tm)))
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
  if (sched_global)
    if (int rc = m.grow_zeroed(&h->tm_sched_scratch, &h->tm_sched_scratch_words, sel.size() * (size_t)scratch_stride))
      return rc;
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
  GF_LAUNCH("cov_tm_schedule_kernel", gf::launch_cov_tm_schedule(t, (int)sel.size(), e_max, h->stream));
  // uint8 entries first (twice the waves per CU); envs it cannot bound get uint16
  GF_LAUNCH("cov_time_matrix_kernel", gf::launch_cov_time_matrix(t, (int)sel.size(), false, h->stream));
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
    GF_LAUNCH("cov_time_matrix_kernel", gf::launch_cov_time_matrix(t, (int)wide.size(), true, h->stream));
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
    greedy_lists(h, t);
    GF_HIP(hipMemcpyAsync(h->tm_envsel, sel.data(), sel.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    GF_LAUNCH("cov_greedy_list_kernel", gf::launch_cov_greedy_lists(t, (int)sel.size(), h->stream));
  }
  GF_HIP(hipStreamSynchronize(h->stream));
  for (int b : sel) h->tm_valid[b] = 1;
  h->tm_ready = true;
  return GF_OK;
}

int gf::ensure_rng_streams(cov_handle* h) {
  if (h->mt_key) return GF_OK;
  const size_t B = h->cfg.n_envs;
  if (int rc = h->mem.zeroed(&h->mt_key, B * gf::kMtN)) return rc;
  return h->mem.zeroed(&h->mt_pos, B);
}

namespace {

// The time matrices current and, where the maps allow them (max_nodes - n_robots <=
// kGreedyListMaxT), the greedy lists present. `refusal`: the call's own GF_EINVAL text
// where they are not (nullptr: the caller has another way). join: cov_step's form, which
// orders `stream` behind everything (use) only when the matrices are rebuilt.
int ensure_greedy_lists(cov_handle* h, const char* refusal, bool join = false) {
  if (!h->tm_ready || !h->tm_glist) {
    if (join)
      if (int rc = use(h)) return rc;
    if (int rc = gf::ensure_time_matrix(h)) return rc;
  }
  if (!h->tm_glist && refusal) return fail(GF_EINVAL, refusal);
  return GF_OK;
}

// controller(greedy=True) in a step's own launch: the greedy lists, the matrices behind
// them and where the actions go (they stay resident); with_rng: the fallback robots draw
// from the envs' np_random streams.
void greedy_args(const cov_handle* h, gf::CovArgs& a, bool with_rng) {
  greedy_lists(h, a);
  a.gcost = h->tm_cost;
  a.gprev = h->tm_prevT;
  a.gactions = h->actions;
  a.needs_random = h->needs_random;
  if (with_rng) {
    a.mt_key = h->mt_key;
    a.mt_pos = h->mt_pos;
  }
}

// The tail of every reset, over the n envs listed on the device in `envs` (nullptr: every
// env): the reset kernel from h->start / h->visited0 (`what` names it in an error), the
// hidden observation's reset, a step with null actions, which makes the observation, and
// its hidden form.
int finish_reset(cov_handle* h, const int32_t* envs, int n, const char* what) {
  GF_LAUNCH(what, envs ? gf::launch_cov_reset_list(h->a, h->start, h->visited0, envs, n, h->stream)
                       : gf::launch_cov_reset(h->a, h->start, h->visited0, h->stream));
  if (int rc = gf::hidden_reset(h, envs, n)) return rc;
  gf::CovArgs a = h->a;
  a.actions = nullptr;
  if (!envs) {
    GF_LAUNCH("cov_step_kernel", gf::launch_cov_step(a, h->stream));
    return gf::hidden_pass(h);
  }
  GF_LAUNCH("cov_step_list_kernel", gf::launch_cov_step_list(a, envs, n, h->stream));
  if (h->hidden) GF_LAUNCH("cov_hidden_list_kernel", gf::launch_cov_hidden_list(hidden_args(h), envs, n, h->stream));
  return GF_OK;
}

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
  if (int rc = finish_reset(h, nullptr, (int)B, "cov_reset_kernel")) return rc;
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
  if (int rc = gf::ensure_rng_streams(h)) return rc;
  gf::CovArgs a = h->a;
  a.mt_key = h->mt_key;
  a.mt_pos = h->mt_pos;
  GF_LAUNCH("cov_reset_seeded",
            gf::launch_cov_seed_reset(a, static_cast<uint32_t>(seed), frac_active, h->start, h->visited0, h->stream));
  if (int rc = finish_reset(h, nullptr, (int)B, "cov_reset_seeded")) return rc;
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
  if (new_maps) {  // the selected envs' next maps, from their own map streams (no flags, a stored configuration)
    const int rcm = sampled ? gf::generate_submaps_sel(h, sel, 0, nullptr, 0, 0, nullptr, nullptr, nullptr)
                            : gf::generate_maps_sel(h, &h->map_cfg, sel, 0, nullptr, 0, nullptr, nullptr, nullptr);
    if (rcm) return rcm;
  }
  if (!h->has_graph) return fail(GF_ESTATE, "set the target graph of every env first (cov_set_targets)");
  gf::DeviceBuffers& m = h->mem;
  int rca;
  if ((rca = gf::ensure_rng_streams(h))) return rca;
  if (!h->rs_envs &&
      ((rca = m.zeroed(&h->rs_envs, B)) || (rca = m.zeroed(&h->rs_ok, B)) || (rca = m.zeroed(&h->rs_region, B * Tm)) ||
       (rca = m.zeroed(&h->rs_status, B)) || (rca = m.zeroed(&h->rs_nregion, B)) ||
       (rca = m.zeroed(&h->rs_start_c, B * R)) || (rca = m.zeroed(&h->rs_visited_c, B * Tm)) ||
       (rca = m.zeroed(&h->rs_region_c, B * Tm))))
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
  GF_LAUNCH("cov_reset_device", gf::launch_cov_reset_draw(d, h->stream));
  if (int rc1 = finish_reset(h, h->rs_ok, nsel, "cov_reset_device")) return rc1;
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
  if (int rc = ensure_greedy_lists(h, "the fused expert needs max_nodes - n_robots <= 1024 (the greedy lists)")) return rc;
  if (int rc = join_s2(h)) return rc;
  gf::CovArgsM m{};
  m.a = h->a;
  m.a.actions = nullptr;
  greedy_args(h, m.a, true);
  m.k_steps = n_steps;
  // both records or neither, whichever the host wants
  const size_t n = (size_t)n_steps * h->cfg.n_envs, want = rewards || done;
  const size_t bytes[2] = {want * n * 8, want * n};
  unsigned char* rec[2];
  if (int rc = gf::scratch_records(h, 2, bytes, rec)) return rc;
  m.reward_k = reinterpret_cast<double*>(rec[0]);
  m.done_k = rec[1];
  GF_LAUNCH("cov_step_multi_kernel", gf::launch_cov_step_multi(m, h->stream));
  h->main_dirty = true;
  h->other_work = true;
  if (!want) return GF_OK;
  if (int rc = copy_out(h, rewards, rec[0], bytes[0])) return rc;
  if (int rc = copy_out(h, done, rec[1], bytes[1])) return rc;
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
    // controller(greedy=True) in the step's own launch, from the greedy lists; without
    // them (Tmax > kGreedyListMaxT) the row-scan greedy kernel, then the step
    const char* refusal = (flags & COV_GREEDY_RNG) ? "COV_GREEDY_RNG needs max_nodes - n_robots <= 1024 (the greedy lists)" : nullptr;
    if (int rc = ensure_greedy_lists(h, refusal, true)) return rc;
    if (!h->tm_glist) {
      if (int rc = cov_controller_greedy(h, nullptr, nullptr, nullptr)) return rc;
      return cov_step(h, nullptr, COV_ACTIONS_RESIDENT);
    }
    a.actions = nullptr;
    greedy_args(h, a, flags & COV_GREEDY_RNG);
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
    GF_LAUNCH("cov_step_kernel", gf::launch_cov_step(a, h->stream));
    GF_LAUNCH("cov_step_kernel", gf::launch_cov_step(a1, h->stream2));
    h->s2_pending = true;
    if (h->timing) h->tw_steps++;
    if (h->hidden) {  // one pass over every env on `stream`, behind both halves and ahead of the next ones
      if (int rc = join_s2(h)) return rc;
      if (int rc = gf::hidden_pass(h)) return rc;
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
  GF_LAUNCH("cov_step_kernel", gf::launch_cov_step(a, h->stream));
  if (int rc = h->hidden ? gf::hidden_pass(h) : GF_OK) return rc;  // in the sampled window: a hidden handle's step pays for it
  if (sample) {
    GF_HIP(hipEventRecord(h->ev[h->ev_used + 1], h->stream));
    h->ev_used += 2;
  }
  if (!(flags & (COV_ACTIONS_DEVICE | COV_ACTIONS_RESIDENT | COV_ACTIONS_GREEDY)))
    GF_HIP(hipStreamSynchronize(h->stream));
  return GF_OK;
}

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
    if (int rc = ensure_greedy_lists(h, "COV_NEXT_GREEDY needs max_nodes - n_robots <= 1024 (the per-node greedy lists)"))
      return rc;
    a.next_greedy = 1;
    greedy_args(h, a, false);  // the next expert actions stay resident as well
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
      if (int rc = h->mem.zeroed(&h->fin_cnt, 1)) return rc;
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
  if (n * 4 <= (size_t)gf::kCovUInlineBytes) {
    GF_LAUNCH("cov_step_kernel", gf::launch_cov_step_uin(a, actions, h->stream));  // actions in the kernel arguments
  } else {
    GF_HIP(hipMemcpyAsync(h->actions, actions, n * 4, hipMemcpyHostToDevice, h->stream));
    a.actions = h->actions;
    GF_LAUNCH("cov_step_kernel", gf::launch_cov_step(a, h->stream));
  }
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
    if (q != hipSuccess) return fail_hip("cov_step_host", q);
  } else {
    // spin on the stream: a drop-in step is latency-bound (a blocking wait's wake-up
    // costs a sizeable part of it)
    for (;;) {
      const hipError_t q = hipStreamQuery(h->stream);
      if (q == hipSuccess) break;
      if (q != hipErrorNotReady) return fail_hip("cov_step_host", q);
    }
  }
  int err = 0;
  for (size_t b = 0; b < B; ++b) err |= h->herr[b];
  if (err) return check_err(h);  // reads, clears and reports the device error word
  return GF_OK;
}

int cov_controller_greedy(cov_handle* h, int32_t* actions, uint8_t* needs_random, int64_t* n_random) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->has_state) return fail(GF_ESTATE, "reset first (cov_reset)");
  if (int rc = use(h)) return rc;
  if (int rc = gf::ensure_time_matrix(h)) return rc;
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
  greedy_lists(h, g);
  GF_LAUNCH("cov_greedy_kernel", gf::launch_cov_greedy(g, h->stream));
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

int cov_get_time_matrix(cov_handle* h, int env, int32_t* cost, int32_t* prev) {
  if (!h || env < 0 || env >= h->cfg.n_envs) return fail(GF_EINVAL, "bad argument");
  if (!h->has_graph) return fail(GF_ESTATE, "set the target graph first (cov_set_targets)");
  if (int rc = use(h)) return rc;
  if (int rc = gf::ensure_time_matrix(h)) return rc;
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
  const char* need_lists = "the fused expert needs max_nodes - n_robots <= 1024 (the greedy lists)";
  if (M - R > gf::kGreedyListMaxT) return fail(GF_EINVAL, need_lists);
  if (int rc = use(h)) return rc;
  if (int rc = ensure_greedy_lists(h, need_lists)) return rc;
  if (int rc = join_s2(h)) return rc;
  gf::CovArgsX x{};
  x.a = h->a;
  x.a.actions = nullptr;
  greedy_args(h, x.a, true);
  x.h = hidden_args(h);
  x.n_steps = n_steps;
  x.record_every = every;
  const size_t B = h->cfg.n_envs, n = (size_t)n_steps * B, K = (size_t)(n_steps / every);
  const size_t L = (size_t)16 * M + 1;
  // device destinations are written in place; host ones go through the scratch
  const bool host = rec && !(rec->flags & COV_ROLLOUT_DEVICE);
  const cov_rollout none{};
  const cov_rollout& r = rec ? *rec : none;
  void* dst[5] = {r.rewards, r.done, r.actions, r.needs_random, r.flat_obs};
  const size_t want[5] = {n * 8, n, n * R * 4, n * R, K * B * L * 4};
  size_t bytes[5];
  for (int k = 0; k < 5; ++k) bytes[k] = host && dst[k] ? want[k] : 0;
  unsigned char* out[5];
  if (int rc = gf::scratch_records(h, 5, bytes, out)) return rc;
  if (!host)
    for (int k = 0; k < 5; ++k) out[k] = static_cast<unsigned char*>(dst[k]);
  x.reward_k = reinterpret_cast<double*>(out[0]);
  x.done_k = out[1];
  x.act_k = reinterpret_cast<int32_t*>(out[2]);
  x.nrand_k = out[3];
  x.flat_k = reinterpret_cast<float*>(out[4]);
  GF_LAUNCH("cov_explore_multi_kernel", gf::launch_cov_explore_multi(x, h->stream));
  h->main_dirty = true;
  h->other_work = true;
  bool fetched = false;
  for (int k = 0; k < 5; ++k)
    if (bytes[k]) {
      if (int rc = copy_out(h, dst[k], out[k], bytes[k])) return rc;
      fetched = true;
    }
  if (!fetched) return GF_OK;
  GF_HIP(hipStreamSynchronize(h->stream));
  return check_err(h);
}

int64_t cov_rollout_lds_bytes(int n_robots, int max_nodes, int auto_reset) {
  if (n_robots < 1 || max_nodes < n_robots) return -1;
  return (int64_t)gf::cov_rollout_lds_layout(n_robots, max_nodes, auto_reset != 0, nullptr);
}

// n_steps fused greedy expert steps with the device fallback draws in one launch, recorded
// (cov_rollout_kernel); with ar, an env whose step sets done is reset inside the launch as
// cov_reset_device(h, {frac_active, nearby, COV_RESET_DONE, 0}, NULL, ...) would reset it.
int cov_expert_rollout(cov_handle* h, int n_steps, const cov_rollout* rec, const cov_auto_reset* ar) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->has_state) return fail(GF_ESTATE, "reset first (cov_reset)");
  if (h->hidden) return fail(GF_EINVAL, std::string("cov_expert_rollout: ") + kHiddenFused);
  if (!h->mt_key) return fail(GF_ESTATE, "set the envs' np_random streams first (cov_set_rng or cov_reset_seeded)");
  if (n_steps < 1) return fail(GF_EINVAL, "n_steps must be at least 1");
  const int every = rec ? rec->record_every : 1;
  if (every < 1 || n_steps % every != 0) return fail(GF_EINVAL, "record_every must be at least 1 and divide n_steps");
  if (rec && (rec->flags & ~COV_ROLLOUT_DEVICE)) return fail(GF_EINVAL, "unknown cov_rollout flags");
  if (ar && ar->flags != 0) return fail(GF_EINVAL, "cov_auto_reset flags must be 0 (no seeding, no new maps inside a launch)");
  if (ar && !(ar->frac_active >= 0.0 && ar->frac_active <= 1.0)) return fail(GF_EINVAL, "frac_active must be in [0, 1]");
  if (ar && ar->nearby < 0) return fail(GF_EINVAL, "nearby must be >= 0");
  const int R = h->cfg.n_robots, M = h->cfg.max_nodes;
  if (R > gf::kMtN) return fail(GF_EINVAL, "n_robots <= 624 (one key regeneration per step)");
  const char* need_lists = "the fused expert needs max_nodes - n_robots <= 1024 (the greedy lists)";
  if (M - R > gf::kGreedyListMaxT) return fail(GF_EINVAL, need_lists);
  const size_t lds = gf::cov_rollout_lds_layout(R, M, ar != nullptr, nullptr);
  if (lds > gf::kCovRolloutLdsMax)
    return fail(GF_EINVAL, "cov_expert_rollout: " + std::to_string(lds) + " bytes of LDS per workgroup exceed 64 KB (cov_rollout_lds_bytes)");
  if (int rc = use(h)) return rc;
  if (int rc = ensure_greedy_lists(h, need_lists)) return rc;
  if (int rc = join_s2(h)) return rc;
  gf::CovArgsR x{};
  x.a = h->a;
  x.a.actions = nullptr;
  greedy_args(h, x.a, true);
  x.n_steps = n_steps;
  x.record_every = every;
  x.auto_reset = ar ? 1 : 0;
  if (ar) {
    x.d.R = R;
    x.d.Tmax = h->a.Tmax;
    x.d.nearby = ar->nearby;
    x.d.frac = ar->frac_active;
    x.d.ntg = h->ntg;
    x.d.nbr = h->a.nbr;
    x.d.cnt = h->a.cnt;
    x.d.mt_key = h->mt_key;
    x.d.mt_pos = h->mt_pos;
    x.d.start = h->start;
    x.d.visited0 = h->visited0;
  }
  const size_t B = h->cfg.n_envs, n = (size_t)n_steps * B, K = (size_t)(n_steps / every);
  const size_t L = (size_t)15 * M + 1;
  // device destinations are written in place; host ones go through the scratch
  const bool device = rec && (rec->flags & COV_ROLLOUT_DEVICE);
  const cov_rollout none{};
  const cov_rollout& r = rec ? *rec : none;
  void* dst[7] = {r.rewards, r.done, r.actions, r.needs_random, r.flat_obs, ar ? ar->n_resets : nullptr,
                  ar ? ar->status : nullptr};
  const size_t want[7] = {n * 8, n, n * R * 4, n * R, K * B * L * 4, B * 4, B * 4};
  size_t bytes[7];
  for (int k = 0; k < 7; ++k) bytes[k] = !device && dst[k] ? want[k] : 0;
  unsigned char* out[7];
  if (int rc = gf::scratch_records(h, 7, bytes, out)) return rc;
  if (device)
    for (int k = 0; k < 7; ++k) out[k] = static_cast<unsigned char*>(dst[k]);
  x.reward_k = reinterpret_cast<double*>(out[0]);
  x.done_k = out[1];
  x.act_k = reinterpret_cast<int32_t*>(out[2]);
  x.nrand_k = out[3];
  x.flat_k = reinterpret_cast<float*>(out[4]);
  x.n_resets = reinterpret_cast<int32_t*>(out[5]);
  x.status = reinterpret_cast<int32_t*>(out[6]);
  GF_LAUNCH("cov_rollout_kernel", gf::launch_cov_rollout(x, h->stream));
  h->main_dirty = true;
  h->other_work = true;
  bool fetched = false;
  for (int k = 0; k < 7; ++k)
    if (bytes[k]) {
      if (int rc = copy_out(h, dst[k], out[k], bytes[k])) return rc;
      fetched = true;
    }
  if (!fetched) return GF_OK;
  GF_HIP(hipStreamSynchronize(h->stream));
  return check_err(h);
}

}  // extern "C"
