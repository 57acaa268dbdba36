// Internal interface of the Coverage-v0 kernels (coverage_kernels.hip) for the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "done_flag.h"
#include "mt19937.h"

namespace gf {

// Device buffers of a batch of B Coverage envs with R robots and room for M nodes
// (robots + targets), i.e. at most Tmax = M - R targets per env.
struct CovArgs {
  int B, R, M, Tmax, episode_length;
  int env0;               // cov_step_kernel: first env of this launch (split steps)
  double res, motion_radius;
  const double* tgt;      // (B,Tmax,2) target positions
  const int32_t* ntg;     // (B) targets per env
  int32_t* nbr;           // (B,Tmax,4) motion-graph neighbours (target-local), -1 padded
  int32_t* cnt;           // (B,Tmax) neighbour counts
  int32_t* n_motion;      // (B) motion edges per env
  double* xr;             // (B,R,2) robot positions
  int32_t* cur;           // (B,R) node each robot is on (global index)
  uint8_t* visited;       // (B,Tmax)
  int32_t* nvisited;      // (B)
  int32_t* step_counter;  // (B)
  uint8_t* dirty;         // (B) robots were placed externally: recompute closest nodes
  const int32_t* actions; // (B,R) in [0,4), or nullptr (observation only)
  double* reward;         // (B)
  uint8_t* done;          // (B)
  float* nodes;           // (B,M,3)
  float* edges;           // (B,4M)
  int32_t* senders;       // (B,4M)
  int32_t* receivers;     // (B,4M)
  int64_t* obs_step;      // (B)
  double* axy;            // (B,Tmax,4,2) coordinates of each node's 4 action targets
  float* nrec;            // (B,Tmax,16) per node, 64 B: its 4 action targets (global, padded
                          // with itself; int4), the 4 action-edge features of a robot on it
                          // (float4), its position (double2), 16 B pad
  int* err;               // device error bits: 1 degree > 4, 2 edges overflow, 4 bad action
  // fused greedy expert (cov_step with COV_ACTIONS_GREEDY): the step's actions are
  // controller(greedy=True)'s, taken from each node's greedy list (below)
  const uint16_t* glist;  // (B,Tmax,gstride) or nullptr: actions come from `actions`
  const uint16_t* glen;   // (B,Tmax)
  int gstride;
  const uint16_t* gcost;  // (B,Tmax,Tmax) hop counts [source][target] (greedy_direct)
  const int16_t* gprev;   // (B,Tmax,Tmax) graph_previous[t, c] at [c][t] (greedy_direct)
  int32_t* gactions;      // (B,R) the greedy actions taken (written)
  uint8_t* needs_random;  // (B,R) robots the reference hands to np_random.choice (action 0 here)
  // COV_GREEDY_RNG: those robots draw np_random.choice(4) (:863-864) from their env's
  // MT19937 stream instead, in robot order, as numpy's legacy RandomState does (nullptr:
  // action 0). The stream is RandomState.get_state()'s key words and position.
  uint32_t* mt_key;       // (B,624)
  int32_t* mt_pos;        // (B) in [0, 624]
  // cov_step_host: after the step, controller(greedy=True)'s actions of the RESULTING state
  // from the greedy lists (glist / glen / gstride) into gactions / needs_random (and the
  // host copies below), for the next step of an expert loop
  int next_greedy;
  // cov_step_host: every output of the env written by the step's own workgroup to page-
  // locked host memory (mapped device addresses) at its end; any may be nullptr
  float* h_nodes;         // (B,M,3)
  float* h_edges;         // (B,4M)
  int32_t* h_senders;     // (B,4M)
  int32_t* h_receivers;   // (B,4M)
  int64_t* h_step;        // (B)
  double* h_reward;       // (B)
  uint8_t* h_done;        // (B)
  int32_t* h_closest;     // (B,R) each robot's node after the step (closest_targets, global)
  int32_t* h_next;        // (B,R) next_greedy actions
  uint8_t* h_nrand;       // (B,R) next_greedy needs_random flags
  int32_t* h_err;         // (B) the device error word as this env's workgroup ends
  DoneFlag fin;           // cov_step_host: the grid's completion flag (done_flag.h)
};

// cov_step_expert: k_steps fused greedy expert steps in one launch, each env's workgroup
// stepping its env k_steps times; step s's rewards and done flags at [s][b] (a separate
// argument block, so the one-step kernel's arguments stay as they are)
struct CovArgsM {
  CovArgs a;
  int k_steps;
  double* reward_k;       // (k_steps,B) or nullptr
  uint8_t* done_k;        // (k_steps,B) or nullptr
};

// cov_step_host: one env's actions travel in the kernel arguments up to this many bytes
constexpr int kCovUInlineBytes = 2048;
struct CovArgsU {
  CovArgs a;
  alignas(16) int32_t u[kCovUInlineBytes / 4];
};

// Greedy lists (built with the time matrix, cov_greedy_list_kernel): for every source
// node c of an env, the targets t with a finite hop count cost[c][t] < MAX_COST, in
// (cost, t) order, i.e. the order of controller(greedy=True)'s np.argmin over the
// masked row (coverage.py:817-819). Entry = t | action << 10 | flag << 12: the index of
// the first hop (graph_previous[t, c], :863-869) among the node's action targets, flag
// 1 when the predecessor is -1 (the reference draws a random action), 2 when it is not
// among them (the reference raises IndexError). Needs Tmax <= 1024.
constexpr int kGreedyListMaxT = 1024;
constexpr uint32_t kGreedyRnd = 1, kGreedyErr = 2;

// The greedy action of a robot on target-local node c from its list row: the first
// entry whose target is unvisited (and is not target 0 once anything is visited: the
// reference masks visited targets through np.where on its (N,1) visited column, which
// also hits column 0). vbits: the env's visited flags as bits (LDS). Returns
// action | flag << 2; flag kGreedyRnd also when every listed target is masked (at once
// when the env has no unvisited target left: nv == T). The row's length and its first
// kGreedyListPad entries are loaded together, and each later round trip brings the next
// kGreedyListPad (four 16-byte loads): late in an episode, when most targets near a robot
// are visited, its scan runs deep into the list, and one 16-byte load per round trip made
// such robots' dependent loads the step's longest phase. Rows are padded to a multiple
// of kGreedyListPad entries (gstride).
constexpr int kGreedyListPad = 32;
__device__ __forceinline__ int greedy_from_list(const uint16_t* row, const uint16_t* lenp, const uint32_t* vbits,
                                                bool any_vis, bool none_left) {
  const uint4* r4 = reinterpret_cast<const uint4*>(row);
  int len = *lenp;
  uint4 q[kGreedyListPad / 8];
#pragma unroll
  for (int c = 0; c < kGreedyListPad / 8; ++c) q[c] = r4[c];
  if (none_left) len = 0;
  for (int k0 = 0; k0 < len; k0 += kGreedyListPad) {
    if (k0 > 0) {
#pragma unroll
      for (int c = 0; c < kGreedyListPad / 8; ++c) q[c] = r4[k0 / 8 + c];
    }
#pragma unroll
    for (int j = 0; j < kGreedyListPad; ++j) {
      const uint4 v = q[j >> 3];
      const uint32_t w = (j & 7) < 2 ? v.x : (j & 7) < 4 ? v.y : (j & 7) < 6 ? v.z : v.w;
      const uint32_t e = (w >> (16 * (j & 1))) & 0xFFFFu;
      const int t = static_cast<int>(e & 1023u);
      const bool masked = ((vbits[t >> 5] >> (t & 31)) & 1u) || (t == 0 && any_vis);
      if (k0 + j < len && !masked) return static_cast<int>(e >> 10);
    }
  }
  return static_cast<int>(kGreedyRnd << 2);
}

// When few targets are left unvisited the list scan runs deep: late in an episode every
// target near a robot is visited and its list's first unvisited entry lies hundreds of
// entries in (a dependent load per 32 entries; 50-80 us steps at config 4). With at most
// kGreedyDirectMax unvisited targets (excluding target 0 once anything is visited, the
// reference's mask) the kernels take the minimum (hop count, target) over that short list
// directly from the robot's cost row instead: the same target, as the list is in that
// order. ulist: the env's unvisited candidates in ascending target order (LDS).
constexpr int kGreedyDirectMax = 32;
constexpr uint32_t kCostInf = 0xFFFF;   // uint16 cost matrix: unreachable
constexpr uint32_t kCostMax = 1000;     // MAX_COST (coverage.py:68)
__device__ __forceinline__ int greedy_direct(const uint16_t* crow, const int16_t* prow, const int32_t* nbr4,
                                             int n, const int* ulist, int U) {
  uint32_t key = 0xFFFFFFFFu;
  for (int k0 = 0; k0 < U; k0 += 8) {  // eight loads of the row in flight
    uint32_t v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = k0 + k < U ? crow[ulist[k0 + k]] : kCostInf;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (v[k] != kCostInf && v[k] < kCostMax) key = min(key, v[k] << 10 | static_cast<uint32_t>(ulist[k0 + k]));
  }
  if (key == 0xFFFFFFFFu) return static_cast<int>(kGreedyRnd << 2);  // every candidate out of reach
  const int t = static_cast<int>(key & 1023u);
  const int p = prow[t];
  if (p < 0) return static_cast<int>(kGreedyRnd << 2);  // :863
  const int4 nb = *reinterpret_cast<const int4*>(nbr4);
  int act = (n > 3 && nb.w == p) ? 3 : 4;  // the first of the node's action targets equal to the next hop
  act = (n > 2 && nb.z == p) ? 2 : act;
  act = (n > 1 && nb.y == p) ? 1 : act;
  act = (n > 0 && nb.x == p) ? 0 : act;
  if (act == 4) return static_cast<int>(kGreedyErr << 2);
  return act;
}
// The candidates of greedy_direct from the visited bits (one wave: lane-ordered ballots
// keep ascending target order); returns their count (<= kGreedyDirectMax is the caller's
// condition: T - visited <= kGreedyDirectMax). Every wave calls it; wave 0 writes.
__device__ __forceinline__ void greedy_direct_list(const uint32_t* vbits, int T, bool any_vis, int* ulist, int* ucount) {
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  int cnt = 0;
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int t = t0 + lane;
    const bool cand = t < T && !((vbits[t >> 5] >> (t & 31)) & 1u) && !(t == 0 && any_vis);
    const uint64_t m = __ballot(cand);
    const int pos = cnt + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                    __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0));
    if (cand && pos < kGreedyDirectMax) ulist[pos] = t;
    cnt += __popcll(m);
  }
  if (lane == 0) *ucount = cnt;
}

// np_random's generator (numpy's legacy RandomState: MT19937, mt19937.h). choice(4) with
// uniform p is randint(0, 4): one 32-bit output, masked to 2 bits (the mask equals the
// range, so no draw is ever rejected).

// RandomState.permutation(n) into perm[0, n) from the stream (key in LDS, pos wave-uniform),
// by one wave (cov_seed_reset_kernel, cov_reset_draw_kernel). The draws do not depend on the
// permutation, so they come first: 64 tempered words per round (one LDS load per lane),
// consumed in stream order by a register chain (readlane; the masked rejection of each i),
// the accepted ones into vseq[i]; then lane 0 runs the swaps, one LDS round trip each (the
// draws and swaps interleaved waited on two per swap; profiles/r06/ab_seed_reset_draws.txt).
// perm and vseq hold n words each. Every lane of the wave calls it. Sync: mt19937.h.
template <class Sync = WgSync>
__device__ __forceinline__ void cov_permute(uint32_t* key, int& pos, int32_t* perm, int32_t* vseq, int n) {
  const Sync sync;
  const int lane = threadIdx.x;
  for (int k = lane; k < n; k += 64) perm[k] = k;
  int i = n - 1;  // wave-uniform
  while (i >= 1) {
    if (pos == kMtN) {
      mt_regen<64, Sync>(key);
      pos = 0;
    }
    const int avail = min(64, kMtN - pos);
    const uint32_t wl = lane < avail ? mt_temper(key[pos + lane]) : 0u;
    int u = 0;
    for (; u < avail && i >= 1; ++u) {
      const uint32_t mask = 0xFFFFFFFFu >> __builtin_clz(static_cast<uint32_t>(i));
      const uint32_t v = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(wl), u)) & mask;
      if (v <= static_cast<uint32_t>(i)) {
        if (lane == 0) vseq[i] = static_cast<int>(v);
        --i;
      }
    }
    pos += u;
  }
  sync();
  if (lane == 0 && n > 1) {  // one lane: its LDS reads and writes stay in program order
    // the next swap's draw is read with this swap's entries (vseq is not written here),
    // so a swap waits on one LDS round trip, not two
    int v = vseq[n - 1];
    for (int k = n - 1; k >= 1; --k) {
      const int vnext = vseq[k - 1];  // vseq[0]: read, never used
      const int t = perm[k];
      const int pv = perm[v];
      perm[k] = pv;
      perm[v] = t;
      v = vnext;
    }
  }
  sync();
}

// Shared by the map kernels (coverage_maps.hip, coverage_arl.hip): workgroup compaction
// and the largest connected component of a radius graph by union-find in LDS.
//
// Exclusive scan of one int per thread over a workgroup of NT threads; *total = the sum.
// wsum: LDS of NT / 64 + 1 ints. Every thread calls it.
template <int NT>
__device__ __forceinline__ int block_exscan(int v, int* wsum, int* total) {
  constexpr int NW = NT / 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int k = 0; k < NW; ++k) {
      const int t = wsum[k];
      wsum[k] = run;
      run += t;
    }
    wsum[NW] = run;
  }
  __syncthreads();
  const int r = wsum[w] + x - v;
  *total = wsum[NW];
  __syncthreads();
  return r;
}

__device__ __forceinline__ int uf_find(volatile int32_t* p, int x) {
  for (int y = p[x]; y != x; y = p[x]) x = y;
  return x;
}

// Joins the trees of a and b: the larger root is hooked under the smaller, so a parent
// is always a lower index and each tree's root is its lowest node.
__device__ __forceinline__ void uf_unite(int32_t* p, int a, int b) {
  for (;;) {
    a = uf_find(p, a);
    b = uf_find(p, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(&p[b], b, a) == b) return;
  }
}

// After every uf_unite (and a barrier): points each of the n nodes at its root, counts
// the components (cnt, zeroed by the caller) and returns the largest as size << 32 |
// (0xFFFFFFFF - root): ties go to the lowest root, argmax(bincount(labels))'s first-label
// rule (scipy numbers components in order of their lowest node). best_s: one LDS word
// zeroed by the caller before its last barrier. Every thread of the NT calls it.
template <int NT>
__device__ __forceinline__ unsigned long long uf_largest(int32_t* parent, int32_t* cnt, int n,
                                                         unsigned long long* best_s) {
  const int tid = threadIdx.x;
  for (int u = tid; u < n; u += NT) {
    const int r = uf_find(parent, u);
    parent[u] = r;
    atomicAdd(&cnt[r], 1);
  }
  __syncthreads();
  unsigned long long key = 0ull;
  for (int u = tid; u < n; u += NT)
    if (parent[u] == u) {
      const unsigned long long k2 = (static_cast<unsigned long long>(cnt[u]) << 32) | (0xFFFFFFFFull - u);
      key = k2 > key ? k2 : key;
    }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(key, d, 64);
    key = o > key ? o : key;
  }
  if ((tid & 63) == 0) atomicMax(best_s, key);
  __syncthreads();
  return *best_s;
}

// Greedy expert (coverage_expert.hip).
struct CovTmArgs {
  int R, M, Tmax, horizon;
  int kcap;                  // flag slots per chunk: horizon+1, or Tmax+1 when unbounded
  int tm_s;                  // sources per wave of the launch: 64, 32, 16 or 8
  int nchunk;                // (Tmax + tm_s - 1) / tm_s
  int t_lds;                 // largest target count among the selected envs
  const int32_t* envs;       // selected envs (blockIdx.y)
  const int32_t* ntg;        // (B)
  const int32_t* n_motion;   // (B)
  const int32_t* senders;    // (B,4M): motion edges first (global indices)
  const int32_t* receivers;  // (B,4M)
  uint8_t* flags;            // (B,nchunk,kcap): bit 0 changed, bit 1 some entry inf
  uint16_t* cost;            // (B,Tmax,Tmax) [source][target], 0xFFFF = inf
  uint8_t* cost8;            // (B,Tmax,Tmax) the same as uint8 (255 = inf), written by the
                             // uint8 pass only (envs whose hop counts all fit)
  int16_t* prevT;            // (B,Tmax,Tmax) [q][source] = graph_previous[source, q]
  uint32_t* sched;           // (B,sched_stride) batched edge schedule
  int32_t* nslots;           // (B) schedule length
  int32_t* nlev;             // (B) schedule levels
  uint8_t* overflow;         // (B) the uint8 pass could not bound an entry: rerun wide
  int sched_stride;
  int32_t* lev_off;          // (B,lev_stride) each level's first schedule slot, then nslots
  int lev_stride;
  int32_t* sched_scratch;    // (n_envs_sel,scratch_stride) the schedule kernel's edges and levels when they
  int scratch_stride;        //   exceed the LDS (4 * e_max + 2 words per selected env), or nullptr: in LDS
  // greedy lists (cov_greedy_list_kernel), when Tmax <= kGreedyListMaxT
  const uint8_t* wide;       // (B) which cost form holds the env's matrix
  const int32_t* nbr;        // (B,Tmax,4)
  const int32_t* cnt;        // (B,Tmax)
  uint16_t* glist;           // (B,Tmax,gstride)
  uint16_t* glen;            // (B,Tmax)
  int gstride;
};

struct CovGreedyArgs {
  int B, R, Tmax;
  const int32_t* ntg;
  const double* tgt;
  const double* xr;
  const uint8_t* dirty;
  const int32_t* cur;
  const uint16_t* cost;
  const uint8_t* cost8;      // used for envs with wide[b] == 0 (half the bytes per row)
  const uint8_t* wide;       // (B) 1: the env's matrix needed uint16 entries
  const int16_t* prevT;
  const uint8_t* visited;
  const int32_t* nvisited;
  const int32_t* nbr;
  const int32_t* cnt;
  int32_t* actions;        // (B,R)
  uint8_t* needs_random;   // (B,R)
  int* err;                // 8: next hop not among the robot's actions
  const uint16_t* glist;   // greedy lists (or nullptr: scan the cost rows)
  const uint16_t* glen;
  int gstride;
};

// the LDS tile of S sources per wave, and the largest S of 64, 32, 16, 8 whose tile fits a
// CU's 160 KB (0: none)
size_t cov_time_matrix_lds_bytes(int t_lds, bool wide, int S);
int cov_time_matrix_sources(int t_lds, bool wide);
// global: the edges and levels in CovTmArgs::sched_scratch, only the columns' state in LDS
size_t cov_tm_schedule_lds_bytes(int t_lds, int e_max, bool global);
hipError_t launch_cov_tm_schedule(const CovTmArgs& a, int n_envs_sel, int e_max, hipStream_t s);
// Pass A + pass B over the selected envs with a.tm_s sources per wave; wide = uint16
// entries (else uint8, which sets overflow[b] for envs it cannot bound).
hipError_t launch_cov_time_matrix(const CovTmArgs& a, int n_envs_sel, bool wide, hipStream_t s);
hipError_t launch_cov_greedy(const CovGreedyArgs& a, hipStream_t s);
// the greedy lists of the selected envs (after their time matrices)
hipError_t launch_cov_greedy_lists(const CovTmArgs& a, int n_envs_sel, hipStream_t s);

// Per-episode target maps (coverage_maps.hip; coverage.py:516-527, make_map.py:30-67,
// :207-231). One workgroup per selected env.
struct CovMapArgs {
  int n_sel;
  const int32_t* envs;       // (n_sel) env of each workgroup
  int R, Tmax;
  int NC;                    // cities per map (<= kMapMaxCities)
  double lo, range;          // cities: lo + range * random_sample (np.random.uniform)
  double road_radius;        // waypoint spacing along each road (motion_radius)
  double near_radius;        // lattice points within it of a waypoint (motion_radius / 1.4)
  double link_radius;        // target radius graph (motion_radius)
  int L;                     // lattice points
  const double2* lat;        // (L) generate_lattice's points, [y, x] columns
  const int32_t* lat_cell;   // (L) each point's cell gi * NJ + gj
  const int32_t* cell;       // (NI * NJ) the lattice point of each cell, or -1
  int NI, NJ, K;             // cell grid, cells searched either side for a link
  int wcap;                  // waypoints the LDS holds
  int G;                     // waypoint grid (G x G cells of side gh from (gx0, gy0)) for the
  double gx0, gy0, gh;       //   near-road test; G = 0: every lattice point scans every waypoint
  double* cities;            // (B, kMapMaxCities, 2): drawn by cov_map_cities_kernel or uploaded
  uint32_t* mt_key;          // (B, 624) each env's map stream (the reference's global np.random)
  int32_t* mt_pos;           // (B)
  uint32_t seed0;            // seed: stream b := RandomState(seed0 + b)
  int seed;
  double* tgt;               // (B, Tmax, 2) out: the largest component's points, lattice order
  int32_t* ntg;              // (B) out: targets (0 when the map is refused)
  int32_t* nraw;             // (B) out: the largest component's size
  int32_t* status;           // (B) out: kMapNearDegenerate | kMapTooMany | kMapTooFew | kMapOverflow
};
constexpr int kMapMaxCities = 32;
constexpr int32_t kMapNearDegenerate = 1, kMapTooMany = 2, kMapTooFew = 4, kMapOverflow = 8;
size_t cov_map_lds_bytes(int L, int wcap, int G);
hipError_t launch_cov_map_cities(const CovMapArgs& a, hipStream_t s);
hipError_t launch_cov_map(const CovMapArgs& a, hipStream_t s);

// CoverageARL-v0 / CoverageFull-v0 (coverage_arl.hip): the target pool of an occupancy
// grid (make_map.py:234-271, coverage_arl.py:46-62), shared by every env of a handle, and
// the per-reset subgraph sampler (coverage_arl.py:64-83).
constexpr int kPoolCap = 8192;  // pool points before the component step (grid_slice10: 1714; 5855 at perimeter_delta 12)
struct CovPoolArgs {
  int n0, n1;                // grid (n0, n1) bytes, nonzero = occupied
  const uint8_t* grid;
  int KP;                    // floor(perimeter_delta): cells searched either side for an occupied cell
  double perimeter_delta;
  double res;                // 0.5 * downsample_rate
  double xmin0, xmin1;       // xyz_min
  int check_connected;
  double link_radius;        // motion_radius
  int K;                     // cells searched either side for a link
  double num_subgraphs;
  int32_t* cell;             // (n0 * n1) cell j * n0 + i -> pool point or -1 (out)
  int32_t* raw_cell;         // (kPoolCap) scratch: cell of each point before the component step
  double2* raw;              // (kPoolCap) scratch: those points
  double2* pool;             // (kPoolCap) out: the pool (all_targets), cell order
  int32_t* pool_cell;        // (kPoolCap) out: each pool point's cell
  double* info;              // (6) out: min_xy, max_xy, subgraph_size
  int32_t* counts;           // (3) out: points before the component step, pool points, overflow flag
};
struct CovSubmapArgs {
  int n_sel;
  const int32_t* envs;       // (n_sel) env of each workgroup
  int R, Tmax;
  int P;                     // pool points
  const double2* pool;       // (P)
  const int32_t* pool_cell;  // (P)
  const int32_t* cell;       // (n0 * n1)
  int n0, n1, K;
  double link_radius;
  double lo_x, lo_y;         // graph_start = lo + range * u (np.random.uniform(low, high))
  double range_x, range_y;
  double sub_x, sub_y;       // subgraph_size: graph_end = graph_start + subgraph_size
  int min_targets, max_tries;
  const double* draws;       // (n_sel, n_draws, 2) given graph_start values, or nullptr: the streams
  int n_draws;
  uint32_t* mt_key;          // (B, 624) each env's map stream (cov_generate_maps' streams)
  int32_t* mt_pos;           // (B)
  uint32_t seed0;
  int seed;
  double* tgt;               // (B, Tmax, 2) out: the accepted component's points, pool order
  int32_t* ntg;              // (B) out: targets (0 when no map was accepted or it is refused)
  int32_t* nraw;             // (B) out: the accepted component's size
  int32_t* status;           // (B) out: kMapTooMany | kMapTooFew | kMapNoWindow
  int32_t* tries;            // (B) out: tries consumed
};
constexpr int32_t kMapNoWindow = 16;
size_t cov_submap_lds_bytes(int P);
hipError_t launch_cov_pool(const CovPoolArgs& a, hipStream_t s);
hipError_t launch_cov_submap(const CovSubmapArgs& a, hipStream_t s);

// The radius test `0 < sqrt(dx*dx + dy*dy) <= r` exactly as np.linalg.norm rounds it, from
// the squared distance s: sqrt is correctly rounded and monotonic, so s at or below r2lo =
// r*r*(1 - 2^-50) always passes and s above r2hi = r*r*(1 + 2^-50) never does (the margins
// exceed the roundings of r*r and of the square root by far); only s between them takes
// the square root. 0 < sqrt(s) iff 0 < s; a NaN s fails both ways.
__device__ __forceinline__ bool within_radius(double s, double r, double r2lo, double r2hi) {
  return s > 0.0 && (s <= r2lo || (s <= r2hi && sqrt(s) <= r));
}

// Hidden-node observation (coverage_hidden.hip; coverage.py:334-346 with hide_nodes=True).
struct CovHiddenArgs {
  int B, R, M, Tmax;
  double radius;             // 4 * DELTA (coverage.py:335)
  const int32_t* ntg;        // (B)
  const double* tgt;         // (B,Tmax,2)
  const double* xr;          // (B,R,2)
  const uint8_t* visited;    // (B,Tmax)
  const float* nodes;        // (B,M,3) the ordinary node rows
  const int32_t* senders;    // (B,4M) the stored senders
  const int32_t* receivers;  // (B,4M)
  const int32_t* n_motion;   // (B)
  uint8_t* discovered;       // (B,M) persistent: 1 robots and discovered targets
  float* hnodes;             // (B,M,4) out: masked rows + the frontier flag
  int32_t* hsenders;         // (B,4M) out: senders, -1 where an end is undiscovered (tail kept)
  uint8_t* gmask;            // (B,Tmax) out: visited | !discovered (the expert's mask)
  int32_t* ngmask;           // (B) out: masked targets
  int32_t* nkeep;            // (B) out: slots of hsenders that are not -1
};
size_t cov_hidden_lds_bytes(int R, int M);
hipError_t launch_cov_hidden(const CovHiddenArgs& a, hipStream_t s);
// the same pass over the n envs listed on the device (an entry < 0 is skipped)
hipError_t launch_cov_hidden_list(const CovHiddenArgs& a, const int32_t* envs, int n, hipStream_t s);
// discovered := robots only, for the n envs listed (envs == nullptr: envs 0..n-1; an entry
// < 0 is skipped)
hipError_t launch_cov_hidden_reset(const CovHiddenArgs& a, const int32_t* envs, int n, hipStream_t s);
// the unpack_obs tuple's edges of the hidden observation (kept slots compacted at off[b])
hipError_t launch_cov_hidden_graphs(const CovHiddenArgs& a, const float* edges_in, const int64_t* off, bool mask_all,
                                    float* edges, int32_t* snd, int32_t* rcv, hipStream_t s);

size_t cov_step_lds_bytes(int R, int M);

// cov_explore_expert: n_steps greedy expert steps of envs that hide nodes in one launch
// (cov_explore_multi_kernel, coverage_kernels.hip), each env's workgroup stepping its env
// n_steps times with the discovered set kept as bits in LDS. a: the step's arguments with the
// greedy lists and the streams set; h: the hidden pass's. Records (any may be nullptr):
// every step's reward, done flag, actions and needs-random flags, and after every
// record_every-th step the env's hidden flat row (cov_flat_obs_kernel's, nf = 4, float32).
struct CovArgsX {
  CovArgs a;
  CovHiddenArgs h;
  int n_steps, record_every;
  int hid_off, tg_off;    // cov_explore_lds_layout's byte offsets into the dynamic LDS
  double* reward_k;       // (n_steps,B)
  uint8_t* done_k;        // (n_steps,B)
  int32_t* act_k;         // (n_steps,B,R)
  uint8_t* nrand_k;       // (n_steps,B,R)
  float* flat_k;          // (n_steps / record_every,B,16M+1)
};
// The kernel's dynamic LDS: the step's region (cov_step_lds_bytes), then from *hid_off the
// hidden pass's (cov_hidden_lds_bytes: robot positions, discovered and frontier bits) with
// four counters, then from *tg_off the env's target positions, which the discovery reads
// every step. Returns the total; the host's guard and the launcher both take it from here.
size_t cov_explore_lds_layout(int R, int M, int* hid_off, int* tg_off);
constexpr size_t kCovExploreLdsMax = 64 * 1024;
hipError_t launch_cov_explore_multi(const CovArgsX& x, hipStream_t s);
// cov_seed_reset_kernel's LDS: the stream's key, the permutation, its draws and the flags
size_t cov_seed_reset_lds_bytes(int Tmax);
// Observation wire formats: the flat FlattenDictWrapper rows (B, (12 + nf) M + 1), nf
// features per row of a.nodes, and the batched unpack_obs graph tuple (edges compacted at
// off[b]).
hipError_t launch_cov_flat_obs(const CovArgs& a, int nf, void* dst, bool f32, hipStream_t s);
hipError_t launch_cov_graphs(const CovArgs& a, const int64_t* off, bool mask_all, float* edges, int32_t* snd,
                             int32_t* rcv, hipStream_t s);
hipError_t launch_cov_graph(const CovArgs& a, const int32_t* envs, int n, hipStream_t s);
hipError_t launch_cov_reset(const CovArgs& a, const int32_t* start, const uint8_t* visited0, hipStream_t s);
// Env-list forms for cov_reset_device (envs on the device, n entries; an entry < 0 is
// skipped): the reset pass and the no-action observation pass of the listed envs only
hipError_t launch_cov_reset_list(const CovArgs& a, const int32_t* start, const uint8_t* visited0, const int32_t* envs,
                                 int n, hipStream_t s);
hipError_t launch_cov_step_list(const CovArgs& a, const int32_t* envs, int n, hipStream_t s);

// cov_reset_device's draws (coverage_reset.hip): one wave per listed env
struct CovResetDrawArgs {
  int n_sel;
  const int32_t* envs;    // (n_sel) env of each wave
  int32_t* envs_ok;       // (n_sel) out: the env, or -1 when it is not to be reset (kResetRegionSmall)
  int R, Tmax;
  int nearby;             // 0: every target may be a start; n > 0: get_n_nearest(choice(T), n)
  int seed;               // 1: the stream of env b starts as RandomState(seed0 + b); 0: continues
  uint32_t seed0;
  double frac;
  const int32_t* ntg;     // (B)
  const int32_t* nbr;     // (B,Tmax,4)
  const int32_t* cnt;     // (B,Tmax)
  uint32_t* mt_key;       // (B,624)
  int32_t* mt_pos;        // (B)
  int32_t* start;         // (B,R) out
  uint8_t* visited0;      // (B,Tmax) out
  uint8_t* region;        // (B,Tmax) out: 1 for the targets of the start region
  int32_t* status;        // (B) out: kResetRegionShort | kResetRegionSmall
  int32_t* nregion;       // (B) out: region nodes
  // the same rows by position in envs (n_sel rows each; any may be nullptr), so a few envs'
  // outputs reach the host in one copy per array
  int32_t* start_c;       // (n_sel,R)
  uint8_t* visited_c;     // (n_sel,Tmax)
  uint8_t* region_c;      // (n_sel,Tmax)
};
constexpr int32_t kResetRegionShort = 1, kResetRegionSmall = 2;
size_t cov_reset_draw_lds_bytes(int Tmax);
hipError_t launch_cov_reset_draw(const CovResetDrawArgs& a, hipStream_t s);
// cov_expert_rollout: n_steps fused greedy expert steps of envs that hide nothing in one
// launch, recorded, with an env that finishes reset inside the launch (cov_rollout_kernel,
// coverage_rollout.hip). a: the step's arguments with the greedy lists and the streams set.
// d (auto_reset only): the draws' arguments; of them R, Tmax, nearby, frac, ntg, nbr, cnt,
// mt_key, mt_pos, start and visited0 are used. Records (any may be nullptr): every step's
// reward, done flag, actions and needs-random flags, and after every record_every-th step the
// env's flat row (cov_flat_obs_kernel's, nf = 3, float32), the row after the reset where one
// has just happened.
struct CovArgsR {
  CovArgs a;
  CovResetDrawArgs d;
  int n_steps, record_every, auto_reset;
  int draw_off;           // cov_rollout_lds_layout's byte offset of the draws' LDS
  double* reward_k;       // (n_steps,B)
  uint8_t* done_k;        // (n_steps,B)
  int32_t* act_k;         // (n_steps,B,R)
  uint8_t* nrand_k;       // (n_steps,B,R)
  float* flat_k;          // (n_steps / record_every,B,15M+1)
  int32_t* n_resets;      // (B) resets of env b made by this launch
  int32_t* status;        // (B) OR of their kResetRegion* bits
};
// The kernel's dynamic LDS: the step's region (cov_step_lds_bytes), then with auto_reset from
// *draw_off the draws' (cov_reset_draw_lds_bytes). Returns the total.
size_t cov_rollout_lds_layout(int R, int M, bool auto_reset, int* draw_off);
constexpr size_t kCovRolloutLdsMax = 64 * 1024;
hipError_t launch_cov_rollout(const CovArgsR& x, hipStream_t s);
// reset()'s random draws on the device for envs seeded seed0 + b (start (B,R), visited0
// (B,Tmax)), the streams left in a.mt_key / a.mt_pos
hipError_t launch_cov_seed_reset(const CovArgs& a, uint32_t seed0, double frac, int32_t* start, uint8_t* visited0,
                                 hipStream_t s);
hipError_t launch_cov_step(const CovArgs& a, hipStream_t s);
hipError_t launch_cov_step_multi(const CovArgsM& m, hipStream_t s);  // m.k_steps steps, one launch
// the step with a.actions read from `u` (host memory, copied into the kernel arguments;
// B * R * 4 <= kCovUInlineBytes)
hipError_t launch_cov_step_uin(const CovArgs& a, const int32_t* u, hipStream_t s);

}  // namespace gf
