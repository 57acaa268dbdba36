// C-ABI of the Coverage-v0 engine, the target maps (include/gymflock.h): cov_set_targets,
// the lattice and cov_generate_maps, the occupancy pool and cov_generate_submaps.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "cov_handle.h"

using namespace gf;  // capi_common.h's helpers and cov_handle.h's internal calls

namespace {

// The shared tail of every call that gave the envs of `sel` (on the device in h->envsel)
// new targets: their motion graphs, the hidden observation's reset, `reads` (the caller's
// own read-backs, enqueued behind them), the device error word, and the host's view of the
// maps: edge counts, target counts (ntg: the device's, as `reads` fetched them; nullptr:
// ntg_host is current), stale time matrices, has_graph.
template <class Reads>
int map_changed(cov_handle* h, const std::vector<int32_t>& sel, const int32_t* ntg, Reads reads) {
  const int B = h->cfg.n_envs;
  GF_LAUNCH("cov_graph_kernel", gf::launch_cov_graph(h->a, h->envsel, (int)sel.size(), h->stream));
  if (int rc = gf::hidden_reset(h, h->envsel, (int)sel.size())) return rc;
  if (int rc = reads()) return rc;
  if (int rc = gf::check_err(h)) return rc;  // synchronises; motion-graph errors (degree > 4, edges)
  GF_HIP(hipMemcpy(h->n_motion_host.data(), h->a.n_motion, B * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int b : sel) {
    if (ntg) h->ntg_host[b] = ntg[b];
    h->tm_valid[b] = 0;
  }
  h->tm_ready = false;
  h->has_graph = true;
  for (int b = 0; b < B; ++b) h->has_graph = h->has_graph && h->ntg_host[b] > 0;
  return GF_OK;
}

// env < 0: every env; else that env
std::vector<int32_t> env_range(const cov_handle* h, int env) {
  std::vector<int32_t> sel;
  const int B = h->cfg.n_envs;
  for (int b = env < 0 ? 0 : env; b < (env < 0 ? B : env + 1); ++b) sel.push_back(b);
  return sel;
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
  GF_HIP(h->mem.free_one(&h->lat));
  GF_HIP(h->mem.free_one(&h->lat_cell));
  GF_HIP(h->mem.free_one(&h->lat_grid));
  std::vector<int32_t> grid((size_t)NI * NJ, -1);
  for (int l = 0; l < L; ++l) grid[cell[l]] = l;
  int rc;
  if ((rc = h->mem.zeroed(&h->lat, (size_t)L)) || (rc = h->mem.zeroed(&h->lat_cell, (size_t)L)) ||
      (rc = h->mem.zeroed(&h->lat_grid, (size_t)NI * NJ)))
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
  gf::DeviceBuffers& m = h->mem;
  int rc;
  if ((rc = m.zeroed(&h->map_key, B * gf::kMtN)) || (rc = m.zeroed(&h->map_pos, B)) ||
      (rc = m.zeroed(&h->map_cities, B * gf::kMapMaxCities * 2)) || (rc = m.zeroed(&h->map_nraw, B)) ||
      (rc = m.zeroed(&h->map_status, B)))
    return rc;
  return GF_OK;
}

}  // namespace

int gf::generate_maps_sel(cov_handle* h, const cov_map_config* mc, const std::vector<int32_t>& sel, uint64_t map_seed,
                          const double* cities, int flags, int32_t* n_targets_out, int32_t* status_out,
                          double* cities_out) {
  const bool given = flags & COV_MAP_CITIES;
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
  if (given) {
    GF_HIP(hipMemcpy2DAsync(h->map_cities + (size_t)b0 * gf::kMapMaxCities * 2, gf::kMapMaxCities * 16, cities,
                            (size_t)NC * 16, (size_t)NC * 16, nsel, hipMemcpyHostToDevice, h->stream));
  } else {
    GF_LAUNCH("cov_map_cities_kernel", gf::launch_cov_map_cities(m, h->stream));
    if (flags & COV_MAP_SEED) h->map_seeded = true;
    h->map_cfg = *mc;
    h->map_cfg_set = true;
  }
  GF_LAUNCH("cov_map_kernel", gf::launch_cov_map(m, h->stream));
  std::vector<int32_t> nraw(B), st(B), ntg(B);
  rc = map_changed(h, sel, ntg.data(), [&]() -> int {
    GF_HIP(hipMemcpyAsync(nraw.data(), h->map_nraw, B * 4, hipMemcpyDeviceToHost, h->stream));
    GF_HIP(hipMemcpyAsync(st.data(), h->map_status, B * 4, hipMemcpyDeviceToHost, h->stream));
    GF_HIP(hipMemcpyAsync(ntg.data(), h->ntg, B * 4, hipMemcpyDeviceToHost, h->stream));
    if (cities_out)
      GF_HIP(hipMemcpy2DAsync(cities_out, (size_t)NC * 16, h->map_cities + (size_t)b0 * gf::kMapMaxCities * 2,
                              gf::kMapMaxCities * 16, (size_t)NC * 16, nsel, hipMemcpyDeviceToHost, h->stream));
    return GF_OK;
  });
  if (rc) return rc;
  std::string bad;
  for (int k = 0; k < nsel; ++k) {
    const int b = sel[k];
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
  if (!bad.empty()) return fail(GF_EINVAL, "cov_generate_maps: " + bad);
  return GF_OK;
}

int gf::generate_submaps_sel(cov_handle* h, const std::vector<int32_t>& sel, uint64_t map_seed, const double* draws,
                             int n_draws, int flags, int32_t* n_targets_out, int32_t* status_out,
                             int32_t* tries_out) {
  const bool given = flags & COV_MAP_DRAWS;
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
    if (int rc = gf::scratch(h, bytes, &d)) return rc;
    GF_HIP(hipMemcpyAsync(d, draws, bytes, hipMemcpyHostToDevice, h->stream));
    m.draws = reinterpret_cast<const double*>(d);
  } else if (flags & COV_MAP_SEED) {
    h->map_seeded = true;
  }
  GF_LAUNCH("cov_submap_kernel", gf::launch_cov_submap(m, h->stream));
  std::vector<int32_t> nraw(B), st(B), tr(B), ntg(B);
  const int rc = map_changed(h, sel, ntg.data(), [&]() -> int {
    GF_HIP(hipMemcpyAsync(nraw.data(), h->map_nraw, B * 4, hipMemcpyDeviceToHost, h->stream));
    GF_HIP(hipMemcpyAsync(st.data(), h->map_status, B * 4, hipMemcpyDeviceToHost, h->stream));
    GF_HIP(hipMemcpyAsync(tr.data(), h->sub_tries, B * 4, hipMemcpyDeviceToHost, h->stream));
    GF_HIP(hipMemcpyAsync(ntg.data(), h->ntg, B * 4, hipMemcpyDeviceToHost, h->stream));
    return GF_OK;
  });
  if (rc) return rc;
  std::string bad;
  for (int k = 0; k < nsel; ++k) {
    const int b = sel[k];
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
  if (!bad.empty()) return fail(GF_EINVAL, "cov_generate_submaps: " + bad);
  return GF_OK;
}

extern "C" {

int cov_set_targets(cov_handle* h, int env, int n_targets, const double* targets) {
  if (!h || !targets) return fail(GF_EINVAL, "null argument");
  const int B = h->cfg.n_envs, Tm = h->a.Tmax;
  if (env >= B) return fail(GF_EINVAL, "env index out of range");
  if (n_targets < 1 || n_targets > Tm)
    return fail(GF_EINVAL, "n_targets must be in [1, max_nodes - n_robots] (PAD_NODES, coverage.py:540-543)");
  if (n_targets < h->cfg.n_robots) return fail(GF_EINVAL, "fewer targets than robots (reset draws distinct starts)");
  if (int rc = use(h)) return rc;
  const std::vector<int32_t> sel = env_range(h, env);
  for (int b : sel) {
    GF_HIP(hipMemcpyAsync(h->tgt + (size_t)b * Tm * 2, targets, (size_t)n_targets * 2 * sizeof(double),
                          hipMemcpyHostToDevice, h->stream));
    h->ntg_host[b] = n_targets;
  }
  GF_HIP(hipMemcpyAsync(h->ntg, h->ntg_host.data(), B * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  GF_HIP(hipMemcpyAsync(h->envsel, sel.data(), sel.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  return map_changed(h, sel, nullptr, [] { return (int)GF_OK; });
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

int cov_generate_maps(cov_handle* h, const cov_map_config* mc, int env, uint64_t map_seed, const double* cities,
                      int flags, int32_t* n_targets_out, int32_t* status_out, double* cities_out) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (int rc = check_map_config(mc)) return rc;
  if (flags & ~(COV_MAP_SEED | COV_MAP_CITIES)) return fail(GF_EINVAL, "flags: COV_MAP_SEED | COV_MAP_CITIES");
  if ((flags & COV_MAP_CITIES) && !cities) return fail(GF_EINVAL, "COV_MAP_CITIES needs the cities");
  if (env >= h->cfg.n_envs) return fail(GF_EINVAL, "env index out of range");
  return gf::generate_maps_sel(h, mc, env_range(h, env), map_seed, cities, flags, n_targets_out, status_out,
                               cities_out);
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
  gf::DeviceBuffers& m = h->mem;
  int rc;
  if (!h->pool_xy) {
    if ((rc = m.zeroed(&h->pool_rawcell, (size_t)gf::kPoolCap)) || (rc = m.zeroed(&h->pool_raw, (size_t)gf::kPoolCap)) ||
        (rc = m.zeroed(&h->pool_cell, (size_t)gf::kPoolCap)) || (rc = m.zeroed(&h->pool_info, (size_t)6)) ||
        (rc = m.zeroed(&h->pool_counts, (size_t)3)) || (rc = m.zeroed(&h->sub_tries, (size_t)h->cfg.n_envs)) ||
        (rc = m.zeroed(&h->pool_xy, (size_t)gf::kPoolCap)))
      return rc;
  }
  h->pool_loaded = false;
  GF_HIP(m.free_one(&h->occ_grid));
  GF_HIP(m.free_one(&h->pool_cellmap));
  if ((rc = m.zeroed(&h->occ_grid, (size_t)n0 * n1)) || (rc = m.zeroed(&h->pool_cellmap, (size_t)n0 * n1))) return rc;
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
  GF_LAUNCH("cov_pool_kernel", gf::launch_cov_pool(p, h->stream));
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

int cov_generate_submaps(cov_handle* h, int env, uint64_t map_seed, const double* draws, int n_draws, int flags,
                         int32_t* n_targets_out, int32_t* status_out, int32_t* tries_out) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (flags & ~(COV_MAP_SEED | COV_MAP_DRAWS)) return fail(GF_EINVAL, "flags: COV_MAP_SEED | COV_MAP_DRAWS");
  if ((flags & COV_MAP_DRAWS) && !draws) return fail(GF_EINVAL, "COV_MAP_DRAWS needs the draws");
  if ((flags & COV_MAP_DRAWS) && n_draws < 1) return fail(GF_EINVAL, "COV_MAP_DRAWS needs n_draws >= 1");
  if ((flags & COV_MAP_DRAWS) && n_draws > (1 << 20)) return fail(GF_EINVAL, "n_draws too large");
  if (env >= h->cfg.n_envs) return fail(GF_EINVAL, "env index out of range");
  return gf::generate_submaps_sel(h, env_range(h, env), map_seed, draws, n_draws, flags, n_targets_out, status_out,
                                  tries_out);
}

}  // extern "C"
