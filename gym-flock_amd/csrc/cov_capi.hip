// C-ABI of the Coverage-v0 engine (include/gymflock.h, cov_* functions): the handle's
// lifecycle, setters and getters, wire formats, streams, timing and hidden nodes. The maps
// are in cov_maps_capi.hip, the resets, steps and experts in cov_step_capi.hip.
#include <cstring>

#include "cov_handle.h"

using namespace gf;  // capi_common.h's helpers and cov_handle.h's internal calls

namespace gf {

int use(cov_handle* h) {
  GF_HIP(hipSetDevice(h->cfg.device));
  if (int rc = join_s2(h)) return rc;
  h->main_dirty = true;
  h->other_work = true;
  return GF_OK;
}

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

int scratch(cov_handle* h, size_t bytes, unsigned char** out) {
  if (bytes > h->scratch_bytes) {
    GF_HIP(h->mem.free_one(&h->scratch));
    h->scratch_bytes = 0;
    if (h->mem.plain(&h->scratch, bytes) != hipSuccess)
      return fail(GF_ENOMEM, "hipMalloc of wire-format scratch failed");
    h->scratch_bytes = bytes;
  }
  *out = h->scratch;
  return GF_OK;
}

int scratch_records(cov_handle* h, int n, const size_t* bytes, unsigned char** rec) {
  const auto padded = [](size_t b) { return (b + 15) & ~(size_t)15; };
  size_t total = 0;
  for (int k = 0; k < n; ++k) total += padded(bytes[k]);
  unsigned char* buf = nullptr;
  if (total)
    if (int rc = scratch(h, total, &buf)) return rc;
  for (int k = 0; k < n; ++k) {
    rec[k] = bytes[k] ? buf : nullptr;
    buf += padded(bytes[k]);
  }
  return GF_OK;
}

// 4 * DELTA (coverage.py:335): the module constant, whatever the env's res
constexpr double kHiddenRadius = 4.0 * 5.5;

CovHiddenArgs hidden_args(const cov_handle* h) {
  CovHiddenArgs g{};
  const CovArgs& a = h->a;
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

int hidden_reset(cov_handle* h, const int32_t* envs, int n) {
  if (h->hidden) GF_LAUNCH("cov_hidden_reset_kernel", launch_cov_hidden_reset(hidden_args(h), envs, n, h->stream));
  return GF_OK;
}

int hidden_pass(cov_handle* h) {
  if (h->hidden) GF_LAUNCH("cov_hidden_kernel", launch_cov_hidden(hidden_args(h), h->stream));
  return GF_OK;
}

}  // namespace gf

namespace {

// The device buffers are `mem`'s; what is left are the streams, the events and the
// page-locked host blocks.
void cov_release(cov_handle* h) {
  if (!h) return;
  hipSetDevice(h->cfg.device);
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->stream2) hipStreamSynchronize(h->stream2);
  h->mem.free_all();
  for (hipEvent_t e : h->ev) hipEventDestroy(e);
  if (h->herr) hipHostFree(h->herr);
  if (h->fin_host) hipHostFree(h->fin_host);
  for (hipEvent_t e : {h->ev_s2, h->ev_main, h->tw[0], h->tw[1]})
    if (e) hipEventDestroy(e);
  if (h->stream) hipStreamDestroy(h->stream);
  if (h->stream2) hipStreamDestroy(h->stream2);
  delete h;
}

// Edge counts of the unpack_obs tuple and their exclusive offsets. On a hidden handle the
// kept slots per env (hnkeep, read from the device: synchronises) replace the motion +
// action edge count.
int graph_sizes(cov_handle* h, bool mask_all, std::vector<int32_t>& ne, std::vector<int64_t>& off) {
  const int B = h->cfg.n_envs, R = h->cfg.n_robots, M = h->cfg.max_nodes;
  std::vector<int32_t> keep;
  if (h->hidden) {
    if (!h->has_state) return fail(GF_ESTATE, "hidden nodes: reset first (the edge counts follow the observation)");
    if (int rc = use(h)) return rc;
    keep.resize(B);
    GF_HIP(hipMemcpyAsync(keep.data(), h->hnkeep, keep.size() * 4, hipMemcpyDeviceToHost, h->stream));
    GF_HIP(hipStreamSynchronize(h->stream));
  }
  ne.assign(B, 0);
  off.assign(B + 1, 0);
  for (int b = 0; b < B; ++b) {
    ne[b] = (mask_all || b == 0) ? (h->hidden ? keep[b] : h->n_motion_host[b] + 8 * R) : 4 * M;
    off[b + 1] = off[b] + ne[b];
  }
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
  gf::DeviceBuffers& m = h->mem;
  if ((rc = m.zeroed(&h->ntg, B)) || (rc = m.zeroed(&h->tgt, B * Tm * 2)) || (rc = m.zeroed(&a.nbr, B * Tm * 4)) ||
      (rc = m.zeroed(&a.cnt, B * Tm)) || (rc = m.zeroed(&a.n_motion, B)) || (rc = m.zeroed(&a.xr, B * R * 2)) ||
      (rc = m.zeroed(&a.cur, B * R)) || (rc = m.zeroed(&a.visited, B * Tm)) || (rc = m.zeroed(&a.nvisited, B)) ||
      (rc = m.zeroed(&a.step_counter, B)) || (rc = m.zeroed(&a.dirty, B)) || (rc = m.zeroed(&h->actions, B * R)) ||
      (rc = m.zeroed(&a.reward, B)) || (rc = m.zeroed(&a.done, B)) || (rc = m.zeroed(&a.nodes, B * M * 3)) ||
      (rc = m.zeroed(&a.edges, B * E)) || (rc = m.zeroed(&a.senders, B * E)) || (rc = m.zeroed(&a.receivers, B * E)) ||
      (rc = m.zeroed(&a.obs_step, B)) || (rc = m.zeroed(&a.axy, B * Tm * 8)) || (rc = m.zeroed(&a.nrec, B * Tm * 16)) ||
      (rc = m.zeroed(&h->err, 1)) || (rc = m.zeroed(&h->start, B * R)) || (rc = m.zeroed(&h->visited0, B * Tm)) ||
      (rc = m.zeroed(&h->envsel, B))) {
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
  if (int rc = gf::ensure_rng_streams(h)) return rc;
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
  GF_LAUNCH("cov_flat_obs_kernel", gf::launch_cov_flat_obs(fa, nf, out, f32, h->stream));
  if (flags & COV_OUT_DEVICE) return GF_OK;  // stream-ordered; cov_sync before reading
  GF_HIP(hipMemcpyAsync(dst, out, bytes, hipMemcpyDeviceToHost, h->stream));
  GF_HIP(hipStreamSynchronize(h->stream));
  return check_err(h);
}

int cov_graphs_tuple_sizes(cov_handle* h, int32_t* n_edge, int64_t* total_edges, int flags) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->has_graph) return fail(GF_ESTATE, "set the target graph first (cov_set_targets)");
  std::vector<int32_t> ne;
  std::vector<int64_t> off;
  if (int rc = graph_sizes(h, flags & COV_MASK_ALL, ne, off)) return rc;
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
  std::vector<int32_t> ne;
  std::vector<int64_t> off;
  if (int rc = graph_sizes(h, flags & COV_MASK_ALL, ne, off)) return rc;
  const int64_t total = off.back();
  if (!h->goff)
    if (h->mem.plain(&h->goff, (B + 1) * sizeof(int64_t)) != hipSuccess)
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
    GF_LAUNCH("cov_graphs_kernel",
              h->hidden ? gf::launch_cov_hidden_graphs(hidden_args(h), h->a.edges, h->goff, flags & COV_MASK_ALL, e_out,
                                                       s_out, r_out, h->stream)
                        : gf::launch_cov_graphs(h->a, h->goff, flags & COV_MASK_ALL, e_out, s_out, r_out, h->stream));
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
    gf::DeviceBuffers& m = h->mem;
    int rc;
    if ((rc = m.zeroed(&h->discovered, B * M)) || (rc = m.zeroed(&h->hnodes, B * M * 4)) ||
        (rc = m.zeroed(&h->hsenders, B * 4 * M)) || (rc = m.zeroed(&h->gmask, B * Tm)) ||
        (rc = m.zeroed(&h->ngmask, B)) || (rc = m.zeroed(&h->hnkeep, B)))
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
