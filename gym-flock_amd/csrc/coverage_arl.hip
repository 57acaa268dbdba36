// HIP kernels (gfx950) for CoverageARL-v0 / CoverageFull-v0: the target pool of an
// occupancy grid and the per-reset subgraph sampler, batched over envs.
//
// Reference: from_occupancy (gym_flock/envs/spatial/make_map.py:234-271), then
// CoverageARLEnv.load_graph (coverage_arl.py:46-62) once per env object, and
// CoverageARLEnv._generate_targets (coverage_arl.py:64-83) in every reset().
//
// cov_pool_kernel (one workgroup, once per handle):
//   1. cells in the order of meshgrid(xs, ys).flatten(): the grid's second index j outer,
//      the first index i inner, reading arr[i, j]; a free cell is kept when its nearest
//      occupied cell is within perimeter_delta: sqrt(di^2 + dj^2) <= perimeter_delta for
//      some occupied cell (the sum is an exact integer and sqrt is correctly rounded and
//      monotone, so the minimum passes exactly when some cell does). Only cells with
//      |di|, |dj| <= floor(perimeter_delta) can pass;
//   2. targets ((cell * res) + xyz_min) + res / 2 per coordinate, rotated (x, y) = (t_y, -t_x);
//   3. with check_connected the largest component of their radius graph 0 < |p - q| <=
//      motion_radius, in cell order (the union-find of coverage_internal.h). Every point is
//      one grid cell, so the candidates of a link are the cells around it; each edge is
//      decided from the f64 coordinates, sqrt(dx * dx + dy * dy) as np.linalg.norm;
//   4. min_xy, max_xy and subgraph_size = (max_xy - min_xy) / num_subgraphs.
//
// cov_submap_kernel (one workgroup per env): tries until a window's largest component
// holds min_targets points. Each try draws graph_start = low + (high - low) * u for x,
// then y (numpy's legacy random_sample from the env's MT19937 stream, or the caller's
// list), keeps the pool points with graph_start <= p < graph_start + subgraph_size in pool
// order; fewer than min_targets: next try (the reference's `continue`); else the largest
// component of their radius graph; fewer than min_targets: next try. The loop is bounded
// by max_tries (streams) or the list's length (kMapNoWindow). The pool is read through
// L2; the window's nodes, the pool -> window map and the union-find forest live in LDS
// (16 bytes per pool point).
#include "coverage_internal.h"

namespace gf {

namespace {

constexpr int kArlThreads = 512;
constexpr int kArlWaves = kArlThreads / 64;

__global__ __launch_bounds__(kArlThreads) void cov_pool_kernel(CovPoolArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int32_t* parent = reinterpret_cast<int32_t*>(smem);  // (kPoolCap) union-find forest
  int32_t* cnt = parent + kPoolCap;                    // (kPoolCap) component sizes by root
  __shared__ int wsum[kArlWaves + 1];
  __shared__ unsigned long long best_s;
  __shared__ double red[kArlWaves][4];
  const int tid = threadIdx.x, n0 = a.n0, n1 = a.n1, NC = n0 * n1;
  if (tid == 0) best_s = 0ull;
  // 1. the kept cells (contiguous chunks per thread keep the cell order)
  const int chunk = (NC + kArlThreads - 1) / kArlThreads;
  const int c0 = min(NC, tid * chunk), c1 = min(NC, c0 + chunk);
  int local = 0;
  for (int c = c0; c < c1; ++c) {
    const int j = c / n0, i = c - j * n0;
    bool keep = false;
    if (!a.grid[(size_t)i * n1 + j]) {
      for (int di = -a.KP; di <= a.KP && !keep; ++di) {
        const int ni = i + di;
        if (ni < 0 || ni >= n0) continue;
        for (int dj = -a.KP; dj <= a.KP && !keep; ++dj) {
          const int nj = j + dj;
          if (nj < 0 || nj >= n1 || !a.grid[(size_t)ni * n1 + nj]) continue;
          keep = sqrt(static_cast<double>(di * di + dj * dj)) <= a.perimeter_delta;
        }
      }
    }
    a.cell[c] = keep ? 1 : 0;
    local += keep ? 1 : 0;
  }
  int nraw;
  int pos = block_exscan<kArlThreads>(local, wsum, &nraw);
  if (nraw > kPoolCap) {
    if (tid == 0) {
      a.counts[0] = nraw;
      a.counts[1] = 0;
      a.counts[2] = 1;
    }
    return;
  }
  // 2. their targets
  const double half = a.res / 2.0;
  for (int c = c0; c < c1; ++c) {
    if (a.cell[c]) {
      const int j = c / n0, i = c - j * n0;
      const double tx = (static_cast<double>(i) * a.res + a.xmin0) + half;
      const double ty = (static_cast<double>(j) * a.res + a.xmin1) + half;
      a.raw[pos] = make_double2(ty, -tx);
      a.raw_cell[pos] = c;
      parent[pos] = pos;
      cnt[pos] = 0;
      a.cell[c] = pos++;
    } else {
      a.cell[c] = -1;
    }
  }
  __syncthreads();
  // 3. the largest component of the radius graph
  int root = -1;
  if (a.check_connected) {
    for (int u = tid; u < nraw; u += kArlThreads) {
      const int c = a.raw_cell[u], j = c / n0, i = c - j * n0;
      const double2 p = a.raw[u];
      for (int dj = -a.K; dj <= a.K; ++dj) {
        const int nj = j + dj;
        if (nj < 0 || nj >= n1) continue;
        for (int di = -a.K; di <= a.K; ++di) {
          const int ni = i + di;
          if (ni < 0 || ni >= n0) continue;
          const int v = a.cell[nj * n0 + ni];
          if (v <= u) continue;  // each pair once
          const double2 q = a.raw[v];
          const double dx = p.x - q.x, dy = p.y - q.y;
          const double r = sqrt(dx * dx + dy * dy);
          if (r > 0.0 && r <= a.link_radius) uf_unite(parent, u, v);
        }
      }
    }
    __syncthreads();
    const unsigned long long best = uf_largest<kArlThreads>(parent, cnt, nraw, &best_s);
    root = static_cast<int>(0xFFFFFFFFull - (best & 0xFFFFFFFFull));
  }
  // the pool: the component's points (or every point) in cell order
  const int rchunk = (nraw + kArlThreads - 1) / kArlThreads;
  const int u0 = min(nraw, tid * rchunk), u1 = min(nraw, u0 + rchunk);
  local = 0;
  for (int u = u0; u < u1; ++u) local += (root < 0 || parent[u] == root) ? 1 : 0;
  int P;
  pos = block_exscan<kArlThreads>(local, wsum, &P);
  double mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
  for (int u = u0; u < u1; ++u) {
    const int c = a.raw_cell[u];
    if (root < 0 || parent[u] == root) {
      const double2 p = a.raw[u];
      a.pool[pos] = p;
      a.pool_cell[pos] = c;
      a.cell[c] = pos++;
      mnx = fmin(mnx, p.x);
      mny = fmin(mny, p.y);
      mxx = fmax(mxx, p.x);
      mxy = fmax(mxy, p.y);
    } else {
      a.cell[c] = -1;
    }
  }
  // 4. min_xy, max_xy, subgraph_size
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mnx = fmin(mnx, __shfl_xor(mnx, d, 64));
    mny = fmin(mny, __shfl_xor(mny, d, 64));
    mxx = fmax(mxx, __shfl_xor(mxx, d, 64));
    mxy = fmax(mxy, __shfl_xor(mxy, d, 64));
  }
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = mnx;
    red[tid >> 6][1] = mny;
    red[tid >> 6][2] = mxx;
    red[tid >> 6][3] = mxy;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kArlWaves; ++w) {
      mnx = fmin(mnx, red[w][0]);
      mny = fmin(mny, red[w][1]);
      mxx = fmax(mxx, red[w][2]);
      mxy = fmax(mxy, red[w][3]);
    }
    a.info[0] = mnx;
    a.info[1] = mny;
    a.info[2] = mxx;
    a.info[3] = mxy;
    a.info[4] = (mxx - mnx) / a.num_subgraphs;
    a.info[5] = (mxy - mny) / a.num_subgraphs;
    a.counts[0] = nraw;
    a.counts[1] = P;
    a.counts[2] = 0;
  }
}

__global__ __launch_bounds__(kArlThreads) void cov_submap_kernel(CovSubmapArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ uint32_t key[kMtN];
  __shared__ int wsum[kArlWaves + 1];
  __shared__ unsigned long long best_s;
  const int e = blockIdx.x;
  if (e >= a.n_sel) return;
  const int b = a.envs[e];
  const int tid = threadIdx.x, P = a.P, n0 = a.n0, n1 = a.n1;
  int32_t* wmap = reinterpret_cast<int32_t*>(smem);  // (P) pool point -> window node or -1
  int32_t* widx = wmap + P;                          // (P) window node -> pool point
  int32_t* parent = widx + P;                        // (P) union-find forest of the window
  int32_t* cnt = parent + P;                         // (P) component sizes by root
  const bool given = a.draws != nullptr;
  int mpos = kMtN;
  if (!given) {
    if (a.seed) {
      if (tid == 0) {
        uint32_t s = a.seed0 + static_cast<uint32_t>(b);
        for (int p = 0; p < kMtN; ++p) {
          key[p] = s;
          s = 1812433253u * (s ^ (s >> 30)) + static_cast<uint32_t>(p + 1);
        }
      }
    } else {
      for (int k = tid; k < kMtN; k += kArlThreads) key[k] = a.mt_key[(size_t)b * kMtN + k];
      mpos = a.mt_pos[b];
    }
  }
  __syncthreads();
  auto next = [&]() {  // every thread runs the same chain (mpos is uniform)
    if (mpos == kMtN) {
      mt_regen<kArlThreads>(key);
      mpos = 0;
    }
    return mt_temper(key[mpos++]);
  };
  auto next_double = [&]() {  // numpy's legacy random_sample
    const uint32_t hi = next() >> 5;
    const uint32_t lo = next() >> 6;
    return (static_cast<double>(hi) * 67108864.0 + static_cast<double>(lo)) / 9007199254740992.0;
  };
  const int chunk = (P + kArlThreads - 1) / kArlThreads;
  const int l0 = min(P, tid * chunk), l1 = min(P, l0 + chunk);
  const int limit = given ? a.n_draws : a.max_tries;
  int tries = 0, T = 0, root = 0;
  bool ok = false;
  while (tries < limit) {
    double gx, gy;
    if (given) {
      const double* d = a.draws + ((size_t)e * a.n_draws + tries) * 2;
      gx = d[0];
      gy = d[1];
    } else {
      const double ux = next_double();
      const double uy = next_double();
      gx = a.lo_x + a.range_x * ux;
      gy = a.lo_y + a.range_y * uy;
    }
    ++tries;
    const double ex = gx + a.sub_x, ey = gy + a.sub_y;
    int local = 0;
    for (int l = l0; l < l1; ++l) {
      const double2 p = a.pool[l];
      const int in = (gx <= p.x && p.x < ex && gy <= p.y && p.y < ey) ? 1 : 0;
      wmap[l] = in;
      local += in;
    }
    int n;
    int w = block_exscan<kArlThreads>(local, wsum, &n);
    if (n < a.min_targets) continue;  // coverage_arl.py:74-75
    for (int l = l0; l < l1; ++l) {
      if (wmap[l]) {
        widx[w] = l;
        parent[w] = w;
        cnt[w] = 0;
        wmap[l] = w++;
      } else {
        wmap[l] = -1;
      }
    }
    if (tid == 0) best_s = 0ull;
    __syncthreads();
    for (int u = tid; u < n; u += kArlThreads) {
      const int l = widx[u];
      const int c = a.pool_cell[l], j = c / n0, i = c - j * n0;
      const double2 p = a.pool[l];
      for (int dj = -a.K; dj <= a.K; ++dj) {
        const int nj = j + dj;
        if (nj < 0 || nj >= n1) continue;
        for (int di = -a.K; di <= a.K; ++di) {
          const int ni = i + di;
          if (ni < 0 || ni >= n0) continue;
          const int l2 = a.cell[nj * n0 + ni];
          if (l2 < 0) continue;
          const int v = wmap[l2];
          if (v <= u) continue;  // each pair once (also: not in the window)
          const double2 q = a.pool[l2];
          const double dx = p.x - q.x, dy = p.y - q.y;
          const double r = sqrt(dx * dx + dy * dy);
          if (r > 0.0 && r <= a.link_radius) uf_unite(parent, u, v);
        }
      }
    }
    __syncthreads();
    const unsigned long long best = uf_largest<kArlThreads>(parent, cnt, n, &best_s);
    T = static_cast<int>(best >> 32);
    root = static_cast<int>(0xFFFFFFFFull - (best & 0xFFFFFFFFull));
    __syncthreads();  // best_s read by every thread before the next try clears it
    if (T >= a.min_targets) {
      ok = true;
      break;
    }
  }
  int fl = 0;
  if (!ok) {
    fl |= kMapNoWindow;
  } else {
    if (T > a.Tmax) fl |= kMapTooMany;
    if (T < a.R) fl |= kMapTooFew;
  }
  if (fl == 0) {  // the component's points in pool order
    int local = 0;
    for (int l = l0; l < l1; ++l) local += (wmap[l] >= 0 && parent[wmap[l]] == root) ? 1 : 0;
    int tot;
    int pos = block_exscan<kArlThreads>(local, wsum, &tot);
    double2* out = reinterpret_cast<double2*>(a.tgt) + (size_t)b * a.Tmax;
    for (int l = l0; l < l1; ++l)
      if (wmap[l] >= 0 && parent[wmap[l]] == root) out[pos++] = a.pool[l];
  }
  if (!given) {
    for (int k = tid; k < kMtN; k += kArlThreads) a.mt_key[(size_t)b * kMtN + k] = key[k];
    if (tid == 0) a.mt_pos[b] = mpos;
  }
  if (tid == 0) {
    a.ntg[b] = fl == 0 ? T : 0;
    a.nraw[b] = ok ? T : 0;
    a.status[b] = fl;
    a.tries[b] = tries;
  }
}

}  // namespace

size_t cov_submap_lds_bytes(int P) { return (size_t)P * 16; }

hipError_t launch_cov_pool(const CovPoolArgs& a, hipStream_t s) {
  const size_t lds = (size_t)kPoolCap * 8;  // parent, cnt
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cov_pool_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cov_pool_kernel, dim3(1), dim3(kArlThreads), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_cov_submap(const CovSubmapArgs& a, hipStream_t s) {
  const size_t lds = cov_submap_lds_bytes(a.P);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cov_submap_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cov_submap_kernel, dim3(a.n_sel), dim3(kArlThreads), lds, s, a);
  return hipGetLastError();
}

}  // namespace gf
