// HIP kernels (gfx950) for gym-flock's Coverage-v0 step, batched over B envs.
//
// Reference (gym_flock/envs/spatial/): coverage.py step :174-204, get_action_edges
// :206-232, _get_obs_reward :234-364, closest_targets :427-432, _initialize_graph
// :529-594; utils.py _get_graph_edges :8-24.
//
// One workgroup per env. Node indices are global as in the reference: robots
// 0..R-1, targets R..R+T-1. The padded graph observation (nodes (M,3), edges (4M,1),
// senders/receivers (4M)) lives in HBM and is updated in place: the motion-graph part
// is written once per graph (cov_graph_kernel), each step rewrites the 8R action
// edges at the tail and flips the "unvisited" feature of newly visited nodes, which
// leaves the arrays equal to what the reference rebuilds every step.
#include <limits.h>

#include <cstring>
#include <type_traits>

#include <hip/hip_runtime.h>

// Phase timeline (diagnostic builds only, -DGF_STAMPS): thread 0 of each workgroup
// records s_memrealtime (100 MHz) at: start (0), first round trip done (1), claims done
// (2), tail writes issued (3), all writes done (4), for scripts/cov_timeline.py.
#ifdef GF_STAMPS
static __device__ unsigned long long gf_cov_stamp_buf[4096 * 8];
#define GF_COV_STAMP(k)                                                              \
  do {                                                                               \
    if (threadIdx.x == 0 && blockIdx.x < 4096)                                       \
      gf_cov_stamp_buf[blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memrealtime();     \
  } while (0)
#else
#define GF_COV_STAMP(k) ((void)0)
#endif

#include "coverage_step.h"

namespace gf {

namespace {

// Motion graph of one env (utils.py:8-24 with self_loops=True, coverage.py:572-594):
// every ordered target pair with 0 < |p_i - p_j| <= radius, in row-major order, which
// per sender is ascending receiver order (what np.where returns in get_action_edges).
// The radius test (within_radius, coverage_internal.h) decides `0 < sqrt(dx*dx + dy*dy) <= r`
// exactly as dist2d rounds it, from the squared distance.

// Targets staged in LDS with a cell grid (GRID, when they fit: cov_graph_lds_bytes): cells of
// side h = radius (1 + 2^-20) over the targets' bounding box, so every target within the
// radius of a node lies in the 3 x 3 cells around it (the margin dwarfs the rounding of the
// cell coordinates); a node's in-radius targets are kept as its 4 smallest indices, the
// row-major scan order of the reference. Without the grid (too many cells, a non-finite
// coordinate, or GRID off) every node scans every target.
constexpr int kGraphCells = 4096;
// GRID's dynamic LDS: the targets, the cells' runs, the targets by cell. It is taken while
// this and the kernel's static arrays (under 2 KB) fit a CU's 160 KB: up to 7,270 targets.
constexpr size_t kGraphLdsMax = 158 * 1024;
constexpr size_t cov_graph_lds_bytes(int Tmax) { return (size_t)Tmax * 20 + (size_t)kGraphCells * 4; }

template <bool GRID>
__global__ __launch_bounds__(kCovThreads) void cov_graph_kernel(CovArgs a, const int32_t* envs, int n_envs_sel) {
  __shared__ int scan[kCovThreads];
  __shared__ int total_s;
  __shared__ double bb_s[kCovThreads / 64][4];
  __shared__ int grid_s[3];  // Gx, Gy (0: scan), cell count
  __shared__ double org_s[2];
  extern __shared__ __attribute__((aligned(16))) double2 tgs[];  // GRID: (Tm) targets, (cells + 1) runs, (Tm) by cell
  const int e = blockIdx.x;
  if (e >= n_envs_sel) return;
  const int b = envs ? envs[e] : e;
  const int R = a.R, M = a.M, Tm = a.Tmax, E = 4 * M;
  const int T = a.ntg[b];
  const double* tg = a.tgt + (size_t)b * Tm * 2;
  int32_t* nbr = a.nbr + (size_t)b * Tm * 4;
  int32_t* cnt = a.cnt + (size_t)b * Tm;
  const int tid = threadIdx.x;
  const double r = a.motion_radius, rr = r * r;
  const double r2lo = rr * (1.0 - 0x1p-50), r2hi = rr * (1.0 + 0x1p-50);
  const double2* tg2 = reinterpret_cast<const double2*>(tg);
  auto test = [&](double px, double py, double2 q) {
    const double dx = px - q.x, dy = py - q.y;
    return within_radius(dx * dx + dy * dy, r, r2lo, r2hi);
  };
  // 1. neighbour lists (<= 4 per node; more is the reference's "Increase MAX_EDGES")
  int Gx = 0, Gy = 0;
  int* cend = reinterpret_cast<int*>(tgs + Tm);  // (cells) end of each cell's run
  int* sidx = cend + kGraphCells;                 // (T) target indices in cell order
  double ox = 0.0, oy = 0.0;
  const double h = r * (1.0 + 0x1p-20);
  if (GRID) {
    double lo_x = __builtin_inf(), lo_y = __builtin_inf(), hi_x = -__builtin_inf(), hi_y = -__builtin_inf();
    bool finite = true;
    for (int j = tid; j < T; j += kCovThreads) {
      const double2 q = tg2[j];
      tgs[j] = q;
      finite = finite && isfinite(q.x) && isfinite(q.y);
      lo_x = fmin(lo_x, q.x), lo_y = fmin(lo_y, q.y), hi_x = fmax(hi_x, q.x), hi_y = fmax(hi_y, q.y);
    }
    if (!finite) lo_x = __builtin_nan("");  // poisons the box: scan
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const double o0 = __shfl_xor(lo_x, d, 64), o1 = __shfl_xor(lo_y, d, 64);
      const double o2 = __shfl_xor(hi_x, d, 64), o3 = __shfl_xor(hi_y, d, 64);
      lo_x = (isnan(o0) || isnan(lo_x)) ? __builtin_nan("") : fmin(lo_x, o0);
      lo_y = fmin(lo_y, o1), hi_x = fmax(hi_x, o2), hi_y = fmax(hi_y, o3);
    }
    if ((tid & 63) == 0) {
      bb_s[tid >> 6][0] = lo_x, bb_s[tid >> 6][1] = lo_y, bb_s[tid >> 6][2] = hi_x, bb_s[tid >> 6][3] = hi_y;
    }
    __syncthreads();
    if (tid == 0) {
      double x0 = bb_s[0][0], y0 = bb_s[0][1], x1 = bb_s[0][2], y1 = bb_s[0][3];
      bool nan = isnan(x0);
      for (int w = 1; w < kCovThreads / 64; ++w) {
        nan = nan || isnan(bb_s[w][0]);
        x0 = fmin(x0, bb_s[w][0]), y0 = fmin(y0, bb_s[w][1]), x1 = fmax(x1, bb_s[w][2]), y1 = fmax(y1, bb_s[w][3]);
      }
      const double fx = (x1 - x0) / h + 1.0, fy = (y1 - y0) / h + 1.0;
      int gx = 0, gy = 0;
      if (!nan && T > 0 && fx < (double)kGraphCells && fy < (double)kGraphCells && fx * fy < (double)kGraphCells) {
        gx = (int)fx, gy = (int)fy;
      }
      grid_s[0] = gx, grid_s[1] = gy;
      org_s[0] = x0, org_s[1] = y0;
    }
    __syncthreads();
    Gx = grid_s[0], Gy = grid_s[1];
    ox = org_s[0], oy = org_s[1];
  }
  // a target's cell: (x - ox) / h >= 0 for every target of the box
  auto cellx = [&](double v) { return min((int)((v - ox) / h), Gx - 1); };
  auto celly = [&](double v) { return min((int)((v - oy) / h), Gy - 1); };
  if (GRID && Gx > 0) {
    const int nc = Gx * Gy;
    for (int c = tid; c < nc; c += kCovThreads) cend[c] = 0;
    __syncthreads();
    for (int j = tid; j < T; j += kCovThreads) atomicAdd(&cend[cellx(tgs[j].x) * Gy + celly(tgs[j].y)], 1);
    __syncthreads();
    if (tid == 0) {  // cell starts (a few thousand cells at most)
      int run = 0;
      for (int c = 0; c < nc; ++c) {
        const int n = cend[c];
        cend[c] = run;
        run += n;
      }
    }
    __syncthreads();
    for (int j = tid; j < T; j += kCovThreads) sidx[atomicAdd(&cend[cellx(tgs[j].x) * Gy + celly(tgs[j].y)], 1)] = j;
    __syncthreads();  // cend[c] is now the end of cell c's run (the start of c + 1)
  }
  for (int i = tid; i < T; i += kCovThreads) {
    const double px = tg[2 * i], py = tg[2 * i + 1];
    int c = 0;
    if (GRID && Gx > 0) {
      // the in-radius targets of the 3 x 3 cells, the 4 smallest indices kept in order
      int n0 = INT_MAX, n1 = INT_MAX, n2 = INT_MAX, n3 = INT_MAX;
      const int ci = cellx(px), cj = celly(py);
      for (int gi = max(ci - 1, 0); gi <= min(ci + 1, Gx - 1); ++gi)
        for (int gj = max(cj - 1, 0); gj <= min(cj + 1, Gy - 1); ++gj) {
          const int cc = gi * Gy + gj, k1 = cend[cc];
          for (int k = cc > 0 ? cend[cc - 1] : 0; k < k1; ++k) {
            const int j = sidx[k];
            if (!test(px, py, tgs[j])) continue;
            ++c;
            int x = j, t;
            t = min(n0, x), x = max(n0, x), n0 = t;
            t = min(n1, x), x = max(n1, x), n1 = t;
            t = min(n2, x), x = max(n2, x), n2 = t;
            n3 = min(n3, x);
          }
        }
      nbr[4 * i] = n0;
      nbr[4 * i + 1] = n1;
      nbr[4 * i + 2] = n2;
      nbr[4 * i + 3] = n3;
    } else {
      for (int j = 0; j < T; ++j) {
        if (test(px, py, GRID ? tgs[j] : tg2[j])) {
          if (c < 4) nbr[4 * i + c] = j;
          ++c;
        }
      }
    }
    if (c > 4) atomicOr(a.err, 1);
    for (int k = c; k < 4; ++k) nbr[4 * i + k] = -1;
    cnt[i] = c > 4 ? 4 : c;
  }
  __syncthreads();
  // 2. exclusive scan of the degrees -> position of each node's edges in the list
  const int per = (T + kCovThreads - 1) / kCovThreads;
  const int i0 = tid * per, i1 = min(T, i0 + per);
  int local = 0;
  for (int i = i0; i < i1; ++i) local += cnt[i];
  scan[tid] = local;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int k = 0; k < kCovThreads; ++k) {
      const int v = scan[k];
      scan[k] = run;
      run += v;
    }
    total_s = run;
  }
  __syncthreads();
  const int n_motion = total_s;
  if (n_motion + 8 * R > E) atomicOr(a.err, 2);
  int32_t* snd = a.senders + (size_t)b * E;
  int32_t* rcv = a.receivers + (size_t)b * E;
  float* edg = a.edges + (size_t)b * E;
  // 3. static observation: motion edges, then -1 / 0 padding
  int off = scan[tid];
  for (int i = i0; i < i1; ++i) {
    for (int k = 0; k < cnt[i]; ++k) {
      const int j = nbr[4 * i + k];
      snd[off] = i + R;
      rcv[off] = j + R;
      edg[off] = static_cast<float>(dist2d(tg[2 * i], tg[2 * i + 1], tg[2 * j], tg[2 * j + 1]));
      ++off;
    }
  }
  for (int k = n_motion + tid; k < E; k += kCovThreads) {
    snd[k] = -1;
    rcv[k] = -1;
    edg[k] = 0.0f;
  }
  float* nodes = a.nodes + (size_t)b * M * 3;
  for (int k = tid; k < M; k += kCovThreads) {
    nodes[3 * k] = k < R ? 1.0f : 0.0f;
    nodes[3 * k + 1] = (k >= R && k < R + T) ? 1.0f : 0.0f;
    nodes[3 * k + 2] = 0.0f;
  }
  // coordinates of every node's 4 action targets (padding = the node itself), so a
  // step reads a moved robot's new action edges in one round trip
  double2* axy = reinterpret_cast<double2*>(a.axy) + (size_t)b * Tm * 4;
  for (int k = tid; k < 4 * T; k += kCovThreads) {
    const int t = k >> 2, ac = k & 3;
    const int q = ac < cnt[t] ? nbr[4 * t + ac] : t;
    axy[k] = make_double2(tg[2 * q], tg[2 * q + 1]);
  }
  // per node, the record a robot moving onto it needs (one 64-byte line): its 4 action
  // targets, the 4 action-edge features from its position (get_action_edges :206-232 with
  // the robot on the node, exactly as the step's full pass computes them) and the position
  float4* rec = reinterpret_cast<float4*>(a.nrec) + (size_t)b * Tm * 4;
  for (int t = tid; t < T; t += kCovThreads) {
    const int c = cnt[t], n = t + R;
    const double px = tg[2 * t], py = tg[2 * t + 1];
    int q[4];
    float d[4];
    for (int k = 0; k < 4; ++k) {
      const int j = k < c ? nbr[4 * t + k] : t;
      q[k] = k < c ? j + R : n;
      d[k] = static_cast<float>(dist2d(px, py, tg[2 * j], tg[2 * j + 1]) / a.res);
    }
    const double2 xy = make_double2(px, py);
    rec[4 * t] = make_float4(__int_as_float(q[0]), __int_as_float(q[1]), __int_as_float(q[2]), __int_as_float(q[3]));
    rec[4 * t + 1] = make_float4(d[0], d[1], d[2], d[3]);
    rec[4 * t + 2] = *reinterpret_cast<const float4*>(&xy);
    rec[4 * t + 3] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (tid == 0) {
    a.n_motion[b] = n_motion;
    a.dirty[b] = 1;  // a new graph: the next pass recomputes nodes and action edges
  }
}

// One step of one env (cov_step_body) and cov_flat_value: coverage_step.h.

template <int NT, bool UIN = false>
__global__ __launch_bounds__(NT) void cov_step_kernel(typename std::conditional<UIN, CovArgsU, CovArgs>::type p) {
  [[maybe_unused]] CovArgs uargs;
  if constexpr (UIN) {
    uargs = p.a;
    uargs.actions = p.u;
  }
  const CovArgs& a = *[&]() -> const CovArgs* {
    if constexpr (UIN) return &uargs;
    else return &p;
  }();
  cov_step_body<NT, false>(a, a.env0 + blockIdx.x, 0, nullptr, nullptr);
#ifdef GF_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  GF_COV_STAMP(4);
#endif
  signal_done(a.fin);  // cov_step_host: the host waits for this, not the stream
}

// cov_step_expert: k_steps steps of every env in one launch, each env's workgroup stepping
// its env k_steps times (the actions come from the device: the greedy lists and the env's
// MT19937 stream), each iteration exactly one cov_step. What an iteration reads of the
// previous one's global writes (robots' nodes, the tail's offers, visited flags, the env's
// words, the key) was written by this workgroup, and the barrier between iterations orders
// it. A kernel of its own: the loop would cost the one-step kernel registers.
template <int NT>
__global__ __launch_bounds__(NT) void cov_step_multi_kernel(CovArgsM p) {
  const int n = p.k_steps > 1 ? p.k_steps : 1;
  for (int it = 0; it < n; ++it) {
    cov_step_body<NT, true>(p.a, p.a.env0 + blockIdx.x, it, p.reward_k, p.done_k);
    __syncthreads();
  }
}

// cov_explore_expert: the expert rollout of envs that hide nodes (ExploreEnv), n_steps
// iterations per workgroup as in cov_step_multi_kernel. The env's discovered set lives as
// bits in LDS for the whole launch (loaded once from the persistent bytes), with the robots'
// and the targets' positions beside it. An iteration is
//   - the greedy step with the expert's mask visited | undiscovered (cov_step_body<HID>: the
//     mask is built from the visited flags, loaded with the robots' loads, and the LDS bits);
//   - this step's actions and needs-random flags into the records;
//   - the hidden pass's own code (cov_hidden_body<KEPT>): discovery from the robots' new
//     positions, which the movers left in LDS (LDS only, but for the byte of each newly
//     discovered target), and, on a recorded iteration and on the last one only, the rest of
//     the pass (the 4M-slot sweep, the node rows, the expert's mask bytes and the counts);
//   - on a recorded iteration the env's flat row from what the workgroup has just written.
// So an iteration that is not recorded has the step's two dependent global round trips and
// no more. What an iteration reads of earlier global writes was written by this workgroup,
// ordered by the barriers (as in cov_step_multi_kernel).
template <int NT>
__global__ __launch_bounds__(NT) void cov_explore_multi_kernel(CovArgsX p) {
  static_assert(NT == kHidThreads, "the hidden pass's loops stride by its own workgroup size");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const CovArgs& a = p.a;
  const CovHiddenArgs& h = p.h;
  const int b = a.env0 + blockIdx.x;
  const int R = a.R, M = a.M, Tm = a.Tmax, W = (M + 31) >> 5;
  const int T = min(a.ntg[b], Tm);
  const int tid = threadIdx.x;
  double2* xr_s = reinterpret_cast<double2*>(smem + p.hid_off);  // (R) robot positions
  uint32_t* dbits = reinterpret_cast<uint32_t*>(xr_s + R);        // (W) discovered
  uint32_t* fbits = dbits + W;                                    // (W) frontier
  int* nm_s = reinterpret_cast<int*>(fbits + W) + 2;              // after the pass's two counters: the expert's count
  double2* tg_s = reinterpret_cast<double2*>(smem + p.tg_off);    // (T) target positions
  const double2* xr = reinterpret_cast<const double2*>(a.xr) + (size_t)b * R;
  const double2* tg = reinterpret_cast<const double2*>(a.tgt) + (size_t)b * Tm;
  uint8_t* disc = h.discovered + (size_t)b * M;
  for (int i = tid; i < R; i += NT) xr_s[i] = xr[i];
  for (int t = tid; t < T; t += NT) tg_s[t] = tg[t];
  for (int w = tid; w < W; w += NT) dbits[w] = hid_robot_word(w, R);
  if (tid == 0) *nm_s = 0;
  __syncthreads();
  for (int t = tid; t < T; t += NT)
    if (disc[R + t]) atomicOr(&dbits[(R + t) >> 5], 1u << ((R + t) & 31));
  __syncthreads();
  const int n = p.n_steps > 1 ? p.n_steps : 1;
  const size_t L = (size_t)16 * M + 1;
  for (int it = 0; it < n; ++it) {
    cov_step_body<NT, true, true>(a, b, it, p.reward_k, p.done_k, dbits, nm_s, xr_s);
    const bool rec = p.flat_k && (it + 1) % p.record_every == 0;
    const size_t row = ((size_t)it * a.B + b) * R;
    if (p.act_k)
      for (int i = tid; i < R; i += NT) p.act_k[row + i] = a.gactions[(size_t)b * R + i];
    if (p.nrand_k)
      for (int i = tid; i < R; i += NT) p.nrand_k[row + i] = a.needs_random[(size_t)b * R + i];
    if (tid == 0) *nm_s = 0;
    // the body's barrier after the moves orders the new positions and its reads of dbits
    cov_hidden_body<true>(h, b, smem + p.hid_off, tg_s, rec || it == n - 1);
    if (rec) {
      __syncthreads();  // the node rows and the hidden senders, written by other waves
      float* out = p.flat_k + ((size_t)((it + 1) / p.record_every - 1) * a.B + b) * L;
      const float* hn = h.hnodes + (size_t)b * M * 4;
      const float* edges = a.edges + (size_t)b * 4 * M;
      const int32_t* hs = h.hsenders + (size_t)b * 4 * M;
      const int32_t* rcv = a.receivers + (size_t)b * 4 * M;
      for (size_t k = tid; k < L; k += NT)
        out[k] = cov_flat_value<float>(k, (size_t)M, (size_t)4 * M, hn, edges, hs, rcv, a.obs_step + b);
    }
    __syncthreads();
  }
}

// cov_reset_device: the observation pass (a.actions == nullptr) of the envs of a device list,
// entries < 0 skipped. A kernel of its own: the step's arguments and code stay as they are.
template <int NT>
__global__ __launch_bounds__(NT) void cov_step_list_kernel(CovArgs a, const int32_t* envs) {
  const int b = envs[blockIdx.x];
  if (b < 0) return;
  cov_step_body<NT, false>(a, b, 0, nullptr, nullptr);
}

// reset (:405-424 after the random draws): robots onto their start targets, the
// unvisited flags, then the same observation pass as a step without actions. envs: the env
// of each workgroup (cov_reset_device; entries < 0 skipped), or nullptr: the workgroup's index.
__global__ __launch_bounds__(kCovThreads) void cov_reset_kernel(CovArgs a, const int32_t* start,
                                                                 const uint8_t* visited0, const int32_t* envs) {
  const int b = envs ? envs[blockIdx.x] : blockIdx.x;
  if (b < 0) return;
  __shared__ int count;
  cov_reset_pass(a, b, start, visited0, &count);  // coverage_step.h
}

// reset()'s draws (coverage.py:405-424) for env b as a reference env whose np_random was
// seeded seed0 + b: RandomState(seed) (mt19937_seed: the generator's init_genrand), then
// choice(arange(T), R, replace=False) for the start targets and choice(arange(T) + R,
// int(T * frac), replace=False) for the unvisited ones, each numpy's legacy permutation of
// the stream (Fisher-Yates from the top, random_interval's masked rejection: oracle/
// mt19937.py). The stream is left in mt_key / mt_pos for the fallback draws
// (COV_GREEDY_RNG). One wave per env: the draws are one chain, which every lane runs, then
// lane 0 swaps; the key regenerations and the tempering take the whole wave.
__global__ __launch_bounds__(64) void cov_seed_reset_kernel(CovArgs a, uint32_t seed0, double frac, int32_t* start,
                                                            uint8_t* visited0) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* key = reinterpret_cast<uint32_t*>(smem);
  int32_t* perm = reinterpret_cast<int32_t*>(key + kMtN);
  int32_t* vseq = perm + a.Tmax;  // [Tm] the draws of one permutation, by i
  uint8_t* vis = reinterpret_cast<uint8_t*>(vseq + a.Tmax);
  const int b = blockIdx.x, lane = threadIdx.x;
  const int R = a.R, Tm = a.Tmax, T = a.ntg[b];
  if (lane == 0) {
    uint32_t s = seed0 + static_cast<uint32_t>(b);
    for (int p = 0; p < kMtN; ++p) {
      key[p] = s;
      s = 1812433253u * (s ^ (s >> 30)) + static_cast<uint32_t>(p + 1);
    }
  }
  __syncthreads();
  int pos = kMtN;  // wave-uniform
  auto permute = [&](int n) { cov_permute(key, pos, perm, vseq, n); };
  permute(T);
  for (int k = lane; k < R; k += 64) start[(size_t)b * R + k] = perm[k];
  __syncthreads();
  permute(T);
  const int kdrop = static_cast<int>(static_cast<double>(T) * frac);  // Python's int(T * frac)
  for (int t = lane; t < Tm; t += 64) vis[t] = 1;
  __syncthreads();
  for (int k = lane; k < kdrop; k += 64) vis[perm[k]] = 0;
  __syncthreads();
  for (int t = lane; t < Tm; t += 64) visited0[(size_t)b * Tm + t] = vis[t];
  for (int k = lane; k < kMtN; k += 64) a.mt_key[(size_t)b * kMtN + k] = key[k];
  if (lane == 0) a.mt_pos[b] = pos;
}

// FlattenDictWrapper order (reference test.py:33, keys coverage.py:90): nodes (M,3),
// edges (4M,1), senders (4M), receivers (4M), step (1,1), concatenated per env. The
// wrapper's np.concatenate promotes to float64; every value here is exact in float32
// too (the Box the wrapper declares), so both widths are offered. nf: features per node
// row of a.nodes (3; 4 with a.nodes / a.senders pointing at the hidden observation).
template <class V>
__global__ __launch_bounds__(kCovThreads) void cov_flat_obs_kernel(CovArgs a, int nf, V* dst) {
  const int b = blockIdx.y;
  const size_t M = a.M, E = 4 * M, N = (size_t)nf * M, L = N + 12 * M + 1;
  V* out = dst + (size_t)b * L;
  const float* nodes = a.nodes + (size_t)b * N;
  const float* edges = a.edges + (size_t)b * E;
  const int32_t* snd = a.senders + (size_t)b * E;
  const int32_t* rcv = a.receivers + (size_t)b * E;
  for (size_t k = (size_t)blockIdx.x * kCovThreads + threadIdx.x; k < L; k += (size_t)gridDim.x * kCovThreads) {
    out[k] = cov_flat_value<V>(k, M, N, nodes, edges, snd, rcv, a.obs_step + b);
  }
}

// unpack_obs (coverage.py:689-741) on the batch: edges, senders and receivers of every
// graph concatenated in env order, node indices offset by b*M, padded edges dropped.
// The reference offsets the senders BEFORE testing them against -1, so only graph 0's
// padding is dropped (a padded sender of graph b > 0 reads b*M - 1); mask_all drops
// every graph's padding instead. Graph b's edges start at off[b].
__global__ __launch_bounds__(kCovThreads) void cov_graphs_kernel(CovArgs a, const int64_t* off, int mask_all,
                                                                 float* edges_out, int32_t* snd_out, int32_t* rcv_out) {
  const int b = blockIdx.y;
  const int M = a.M, E = 4 * M, tail0 = E - 8 * a.R;
  const int nm = a.n_motion[b];
  const bool keep_all = !mask_all && b > 0;
  const float* edges = a.edges + (size_t)b * E;
  const int32_t* snd = a.senders + (size_t)b * E;
  const int32_t* rcv = a.receivers + (size_t)b * E;
  const int64_t base = off[b];
  const int32_t shift = b * M;
  for (int k = blockIdx.x * kCovThreads + threadIdx.x; k < E; k += gridDim.x * kCovThreads) {
    int64_t dst;
    if (keep_all || k < nm)
      dst = base + k;
    else if (k >= tail0)
      dst = base + nm + (k - tail0);
    else
      continue;  // padding (sender -1)
    edges_out[dst] = edges[k];
    snd_out[dst] = snd[k] + shift;
    rcv_out[dst] = rcv[k] + shift;
  }
}

}  // namespace

hipError_t launch_cov_flat_obs(const CovArgs& a, int nf, void* dst, bool f32, hipStream_t s) {
  const size_t L = (size_t)(12 + nf) * a.M + 1;
  const dim3 grid((unsigned)((L + 4 * kCovThreads - 1) / (4 * kCovThreads)), a.B);
  if (f32)
    hipLaunchKernelGGL(cov_flat_obs_kernel<float>, grid, dim3(kCovThreads), 0, s, a, nf, static_cast<float*>(dst));
  else
    hipLaunchKernelGGL(cov_flat_obs_kernel<double>, grid, dim3(kCovThreads), 0, s, a, nf, static_cast<double*>(dst));
  return hipGetLastError();
}

hipError_t launch_cov_graphs(const CovArgs& a, const int64_t* off, bool mask_all, float* edges, int32_t* snd,
                             int32_t* rcv, hipStream_t s) {
  const int E = 4 * a.M;
  const dim3 grid((unsigned)((E + 4 * kCovThreads - 1) / (4 * kCovThreads)), a.B);
  hipLaunchKernelGGL(cov_graphs_kernel, grid, dim3(kCovThreads), 0, s, a, off, mask_all ? 1 : 0, edges, snd, rcv);
  return hipGetLastError();
}

size_t cov_step_lds_bytes(int R, int M) {
  return (size_t)3 * R * 4 + (size_t)2 * ((M + 31) / 32) * 4 + 16 + (size_t)M * 4 + (size_t)((M - R + 63) / 64) * 8 +
         (size_t)(kGreedyDirectMax + 1) * 4 + (size_t)kMtN * 4 + (size_t)((R + 63) / 64) * 8;
}

hipError_t launch_cov_graph(const CovArgs& a, const int32_t* envs, int n, hipStream_t s) {
  if (cov_graph_lds_bytes(a.Tmax) <= kGraphLdsMax) {
    const size_t lds = cov_graph_lds_bytes(a.Tmax);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cov_graph_kernel<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cov_graph_kernel<true>, dim3(n), dim3(kCovThreads), lds, s, a, envs, n);
  } else {
    hipLaunchKernelGGL(cov_graph_kernel<false>, dim3(n), dim3(kCovThreads), 0, s, a, envs, n);
  }
  return hipGetLastError();
}

size_t cov_seed_reset_lds_bytes(int Tmax) { return (size_t)kMtN * 4 + (size_t)Tmax * 9; }

hipError_t launch_cov_seed_reset(const CovArgs& a, uint32_t seed0, double frac, int32_t* start, uint8_t* visited0,
                                 hipStream_t s) {
  const size_t lds = cov_seed_reset_lds_bytes(a.Tmax);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cov_seed_reset_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cov_seed_reset_kernel, dim3(a.B), dim3(64), lds, s, a, seed0, frac, start, visited0);
  return hipGetLastError();
}

hipError_t launch_cov_reset(const CovArgs& a, const int32_t* start, const uint8_t* visited0, hipStream_t s) {
  hipLaunchKernelGGL(cov_reset_kernel, dim3(a.B), dim3(kCovThreads), 0, s, a, start, visited0,
                     static_cast<const int32_t*>(nullptr));
  return hipGetLastError();
}

hipError_t launch_cov_reset_list(const CovArgs& a, const int32_t* start, const uint8_t* visited0, const int32_t* envs,
                                 int n, hipStream_t s) {
  hipLaunchKernelGGL(cov_reset_kernel, dim3(n), dim3(kCovThreads), 0, s, a, start, visited0, envs);
  return hipGetLastError();
}

hipError_t launch_cov_step_list(const CovArgs& a, const int32_t* envs, int n, hipStream_t s) {
  hipLaunchKernelGGL(cov_step_list_kernel<kCovThreads>, dim3(n), dim3(kCovThreads), cov_step_lds_bytes(a.R, a.M), s, a,
                     envs);
  return hipGetLastError();
}

hipError_t launch_cov_step_uin(const CovArgs& a, const int32_t* u, hipStream_t s) {
  const size_t bytes = (size_t)a.B * a.R * 4;
  if (bytes > (size_t)kCovUInlineBytes || !u) return hipErrorInvalidValue;
  CovArgsU p;
  p.a = a;
  p.a.actions = nullptr;
  std::memcpy(p.u, u, bytes);
  void* args[] = {&p};
  return hipLaunchKernel(reinterpret_cast<const void*>(&cov_step_kernel<kCovThreads, true>), dim3(a.B),
                         dim3(kCovThreads), args, cov_step_lds_bytes(a.R, a.M), s);
}

hipError_t launch_cov_step_multi(const CovArgsM& m, hipStream_t s) {
  void* args[] = {const_cast<CovArgsM*>(&m)};
  return hipLaunchKernel(reinterpret_cast<const void*>(&cov_step_multi_kernel<kCovThreads>), dim3(m.a.B),
                         dim3(kCovThreads), args, cov_step_lds_bytes(m.a.R, m.a.M), s);
}

size_t cov_explore_lds_layout(int R, int M, int* hid_off, int* tg_off) {
  const size_t hid = (cov_step_lds_bytes(R, M) + 15) & ~(size_t)15;
  const size_t tg = (hid + cov_hidden_lds_bytes(R, M) + 16 + 15) & ~(size_t)15;
  if (hid_off) *hid_off = (int)hid;
  if (tg_off) *tg_off = (int)tg;
  return tg + (size_t)(M - R) * 16;
}

hipError_t launch_cov_explore_multi(const CovArgsX& x, hipStream_t s) {
  CovArgsX p = x;
  const size_t lds = cov_explore_lds_layout(p.a.R, p.a.M, &p.hid_off, &p.tg_off);
  if (lds > kCovExploreLdsMax) return hipErrorInvalidValue;
  void* args[] = {&p};
  return hipLaunchKernel(reinterpret_cast<const void*>(&cov_explore_multi_kernel<kCovThreads>), dim3(p.a.B),
                         dim3(kCovThreads), args, lds, s);
}

hipError_t launch_cov_step(const CovArgs& a, hipStream_t s) {
  // hipLaunchKernel with the argument pointer: the step is host-bound at two launches
  // per step, and the hipLaunchKernelGGL wrapper's repacking measured ~0.15 us more per
  // launch (scripts/graphprobe.hip)
  void* args[] = {const_cast<CovArgs*>(&a)};
  return hipLaunchKernel(reinterpret_cast<const void*>(&cov_step_kernel<kCovThreads>), dim3(a.B), dim3(kCovThreads),
                         args, cov_step_lds_bytes(a.R, a.M), s);
}

#ifdef GF_STAMPS
extern "C" __attribute__((visibility("default"))) int cov_diag_stamps(unsigned long long* dst, int n) {
  if (n > 4096 * 8) n = 4096 * 8;
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(gf_cov_stamp_buf), (size_t)n * 8, 0, hipMemcpyDeviceToHost) == hipSuccess
             ? 0
             : -1;
}
#endif

}  // namespace gf
