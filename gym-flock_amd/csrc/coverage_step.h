// One step of one Coverage env by its workgroup (cov_step_body) and the passes that go with it
// (the reset pass, an element of the flat row), as device functions, so that the kernels of
// coverage_kernels.hip and the recorded rollout with in-launch resets (coverage_rollout.hip)
// run the same code. coverage_kernels.hip has the account of the data layout.
#pragma once
#include <limits.h>

#include <type_traits>

#include "coverage_hidden.h"
#include "coverage_internal.h"

// Phase timeline stamps: coverage_kernels.hip defines the macro in its diagnostic build
#ifndef GF_COV_STAMP
#define GF_COV_STAMP(k) ((void)0)
#endif

namespace gf {

constexpr int kCovThreads = 256;

__device__ __forceinline__ double dist2d(double ax, double ay, double bx, double by) {
  const double dx = ax - bx, dy = ay - by;
  return sqrt(dx * dx + dy * dy);  // np.linalg.norm of a 2-vector: sqrt(dx*dx + dy*dy)
}

// Action targets of a robot on node c (global): its out-neighbours, padded with c.
__device__ __forceinline__ int action_node(const int32_t* nbr, const int32_t* cnt, int c, int act, int R) {
  const int t = c - R;
  return act < cnt[t] ? nbr[4 * t + act] + R : c;
}

// One step (or, with a.actions == nullptr, the observation that reset() returns).
//
// Two dependent global round trips per env. (1) Each robot's node, action, and the 4
// action targets its node offers: the observation tail written by the previous pass
// already lists them (coverage.py:206-232), so the chosen node needs no neighbour
// lookup. (2) After the LDS-only claim resolution, each robot that moved reads its new
// node's position, visited flag, neighbours and their coordinates (cov_graph_kernel's
// table) together, and rewrites its 8 tail edges; a robot that stayed keeps its edges.
// After an external placement, a new graph or a reset, everything is recomputed.
// UIN (cov_step_host): the env batch's actions arrive in the kernel arguments (CovArgsU)
// instead of being read from memory, one dependent round trip fewer.
// One step of env b (a.env0 + blockIdx.x in the kernels below, an entry of a device list in
// cov_step_list_kernel): MULTI also records the step's
// reward and done flag at [it][b] of reward_k / done_k.
// HID (cov_explore_multi_kernel, a greedy step of an env that hides nodes): the expert masks
// the targets that are visited OR undiscovered (controller :817-821; dbits: the env's
// discovered set as node bits in LDS), and their count, summed into *nm_s (zero on entry)
// by the waves that build the mask, stands where the visited count decides how the expert
// picks; a robot that moves also leaves its new position in xr_lds[i].
template <int NT, bool MULTI, bool HID = false>
__device__ __forceinline__ void cov_step_body(const CovArgs& a, const int b, [[maybe_unused]] int it,
                                              [[maybe_unused]] double* reward_k, [[maybe_unused]] uint8_t* done_k,
                                              [[maybe_unused]] const uint32_t* dbits = nullptr,
                                              [[maybe_unused]] int* nm_s = nullptr,
                                              [[maybe_unused]] double2* xr_lds = nullptr) {
  constexpr int RPT = kCovThreads / NT;  // robots per thread when R <= kCovThreads
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int R = a.R, M = a.M, Tm = a.Tmax, E = 4 * M;
  const int T = a.ntg[b];
  int* cur_s = reinterpret_cast<int*>(smem);          // R: node before the move
  int* new_s = cur_s + R;                             // R: node after the move
  int* chosen = new_s + R;                            // R: node the action points at
  unsigned* claim = reinterpret_cast<unsigned*>(chosen + R);  // (M+31)/32 claim bits
  unsigned* seen = claim + (M + 31) / 32;                      // visited-this-step bits
  int* counter = reinterpret_cast<int*>(seen + (M + 31) / 32);
  int* first = counter + 4;                                    // M: first claimer of each node
  uint32_t* gvis = reinterpret_cast<uint32_t*>(first + M);     // greedy: visited bits, 64 per 2 words
  int* ulist = reinterpret_cast<int*>(gvis + ((a.Tmax + 63) / 64) * 2);  // greedy_direct candidates
  int* ucount = ulist + kGreedyDirectMax;
  const int W = (M + 31) / 32;
  const int tid = threadIdx.x;
  const double* tg = a.tgt + (size_t)b * Tm * 2;
  const int32_t* nbr = a.nbr + (size_t)b * Tm * 4;
  const int32_t* cnt = a.cnt + (size_t)b * Tm;
  const double2* axy = reinterpret_cast<const double2*>(a.axy) + (size_t)b * Tm * 4;
  double* xr = a.xr + (size_t)b * R * 2;
  int32_t* cur = a.cur + (size_t)b * R;
  uint8_t* vis = a.visited + (size_t)b * Tm;
  int32_t* snd = a.senders + (size_t)b * E;
  int32_t* rcv = a.receivers + (size_t)b * E;
  float* edg = a.edges + (size_t)b * E;
  const int base = E - 8 * R;  // action edges: [base, base+4R) target->robot, then robot->target

  for (int k = tid; k < W; k += NT) {
    claim[k] = 0u;
    seen[k] = 0u;
  }
  if (a.actions || a.glist)
    for (int k = tid; k < M; k += NT) first[k] = INT_MAX;
  if (tid == 0) {
    counter[0] = 0;  // targets newly visited
    counter[1] = 0;  // COV_GREEDY_RNG: fallback robots
  }
  GF_COV_STAMP(0);
  const int32_t* act = a.actions ? a.actions + (size_t)b * R : nullptr;
  // COV_ACTIONS_GREEDY: controller(greedy=True) picks each robot's action in this launch
  const bool greedy = a.glist != nullptr && !a.next_greedy;
  const bool has_act = act || greedy;
  // One robot per thread (R <= NT): the data of the node a robot will end on
  // (if it moves: the chosen node; in a full pass: its node) is loaded right after the
  // chosen node is known, so that round trip runs under the claim resolution.
  const bool one = R <= kCovThreads;
  const float4* rec = reinterpret_cast<const float4*>(a.nrec) + (size_t)b * Tm * 4;
  // per robot slot: the chosen node's record (n = -1: none)
  struct Pf {
    int n;
    float4 r0, r1, r2;
    uint8_t was;
  };
  Pf pf[RPT];
  // a robot that stays in a full pass keeps its own position (xr, which after an external
  // placement need not be its node's): its edges come from the coordinate table
  auto load_node = [&](int t, uint8_t& was, int4& q4, int& nc, double2& c0, double2& c1, double2& c2,
                       double2& c3) {
    was = vis[t];
    q4 = *reinterpret_cast<const int4*>(nbr + 4 * t);
    nc = cnt[t];
    c0 = axy[4 * t];
    c1 = axy[4 * t + 1];
    c2 = axy[4 * t + 2];
    c3 = axy[4 * t + 3];
  };
  // robot i's loads: the node, the action and the 4 action targets offered at the node, i.e.
  // the tail of the last observation, read whether or not the env is dirty so that it is
  // not a dependent load
  struct Ld {
    int c, ai;
    int4 offer;
  };
  auto load = [&](int i) {
    Ld l;
    l.c = cur[i];
    l.ai = act ? act[i] : 0;
    l.offer = has_act ? *reinterpret_cast<const int4*>(snd + base + 4 * i) : make_int4(0, 0, 0, 0);
    return l;
  };
  Ld ld[RPT];  // R <= kCovThreads: every slot's loads issued first, before the env's words
  if (one) {
#pragma unroll
    for (int j = 0; j < RPT; ++j)
      if (tid + j * NT < R) ld[j] = load(tid + j * NT);
  }
  // the env's words, loaded up front so none of them costs a round trip of its own
  // COV_GREEDY_RNG: the env's MT19937 key, loaded now with the robots' loads (its words
  // are only written by this workgroup, below) so the fallback draws after the picks do
  // not wait for a global round trip of their own
  constexpr int kKeyPer = (kMtN + NT - 1) / NT;
  uint32_t kpre[kKeyPer];
  const bool rng_pre = a.glist != nullptr && !a.next_greedy && a.mt_key != nullptr;
  if (rng_pre) {
#pragma unroll
    for (int j = 0; j < kKeyPer; ++j) {
      const int k = tid + j * NT;
      kpre[j] = k < kMtN ? a.mt_key[(size_t)b * kMtN + k] : 0u;
    }
  }
  const bool dirty = a.dirty[b] != 0;
  const int nv0 = a.nvisited[b], sc0 = a.step_counter[b];
  const bool full = dirty || !has_act;  // recompute every robot's action edges
  bool any_vis = nv0 > 0;
  int nmask = nv0;  // the targets the expert masks
  if (greedy || a.next_greedy) {
    // the env's visited flags as bits, before this step marks any (ballots, no atomics),
    // read after the robots' loads are in flight
    const int lane = tid & 63, wv = tid >> 6;
    [[maybe_unused]] int nm_w = 0;
    for (int t0 = wv * 64; t0 < Tm; t0 += NT) {
      const int t = t0 + lane;
      uint64_t m;
      if constexpr (HID) {
        m = __ballot(t < T && (vis[t] || !hid_bit(dbits, R + t)));
        nm_w += __popcll(m);
      } else {
        m = __ballot(t < T && vis[t]);
      }
      if (lane == 0) {
        gvis[t0 >> 5] = static_cast<uint32_t>(m);
        gvis[(t0 >> 5) + 1] = static_cast<uint32_t>(m >> 32);
      }
    }
    if constexpr (HID) {
      if (lane == 0 && nm_w) atomicAdd(nm_s, nm_w);
    }
    if (rng_pre) {  // the prefetched key into its LDS words (read by the draws below)
      uint32_t* kb = reinterpret_cast<uint32_t*>(ulist + kGreedyDirectMax + 1);
#pragma unroll
      for (int j = 0; j < kKeyPer; ++j)
        if (tid + j * NT < kMtN) kb[tid + j * NT] = kpre[j];
    }
    __syncthreads();
    if constexpr (HID) {  // the reference's column-0 quirk follows the joined mask
      nmask = *nm_s;
      any_vis = nmask > 0;
    }
  }
  // few targets left unvisited: the greedy actions from the short candidate list
  const bool gdirect = greedy && T - nmask <= kGreedyDirectMax;
  if (gdirect) {
    greedy_direct_list(gvis, T, any_vis, ulist, ucount);
    __syncthreads();
  }
  // the node action ai of a robot on c points at (:184-200)
  auto aim = [&](int c, int ai, const int4& offer) {
    return dirty ? action_node(nbr, cnt, c, ai, R)
                 : (ai == 0 ? offer.x : ai == 1 ? offer.y : ai == 2 ? offer.z : offer.w);
  };
  auto prefetch = [&](Pf& p, int n) {
    const int t = n - R;
    p.n = n;
    p.r0 = rec[4 * t];
    p.r1 = rec[4 * t + 1];
    p.r2 = rec[4 * t + 2];
    p.was = vis[t];
  };
  // robot i: its node c and the node n its action points at (claiming c if n == c)
  auto pick = [&](int i, const Ld& l, int& c) {
    c = l.c;
    int ai = l.ai;
    const int4 offer = l.offer;
    if (dirty) {
      // closest_targets (:427-432): the robots were placed externally
      const double px = xr[2 * i], py = xr[2 * i + 1];
      double best = __builtin_inf();
      c = 0;
      for (int j = 0; j < T; ++j) {
        const double d = dist2d(px, py, tg[2 * j], tg[2 * j + 1]);
        if (d < best) {  // strict: first index on ties, like np.argmin
          best = d;
          c = j;
        }
      }
      c += R;
    }
    cur_s[i] = c;
    int n = c;
    if (greedy) {  // :814-869 from the node's greedy list; fallbacks: action 0 or drawn below
      const size_t row = (size_t)b * Tm + (c - R);
      const int g = gdirect ? greedy_direct(a.gcost + row * Tm, a.gprev + row * Tm, nbr + 4 * (c - R), cnt[c - R],
                                            ulist, *ucount)
                            : greedy_from_list(a.glist + row * a.gstride, a.glen + row, gvis, any_vis, nmask >= T);
      const uint32_t flag = static_cast<uint32_t>(g) >> 2;
      if (flag & kGreedyErr) atomicOr(a.err, 8);
      const bool rnd = flag & kGreedyRnd;
      ai = rnd ? 0 : (g & 3);
      a.needs_random[(size_t)b * R + i] = rnd ? 1 : 0;
      if (rnd && a.mt_key) {  // COV_GREEDY_RNG: drawn in robot order after every pick
        chosen[i] = -1;
        atomicAdd(counter + 1, 1);
        return c;
      }
      a.gactions[(size_t)b * R + i] = ai;
    }
    if (has_act) {
      // step (:184-200): the node the action points at; robots that stay claim first
      if (ai < 0 || ai >= 4) {
        atomicOr(a.err, 4);
        ai = 0;
      }
      n = aim(c, ai, offer);
      chosen[i] = n;
      if (n == c) atomicOr(&claim[n >> 5], 1u << (n & 31));
    }
    return n;
  };
  if (one) {
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
      pf[j].n = -1;
      const int i = tid + j * NT;
      if (i < R) {
        int c;
        const int n = pick(i, ld[j], c);
        if (n != c) pf[j].n = n;
      }
    }
    // then every slot's record: no wait for one slot's record before the next slot
#pragma unroll
    for (int j = 0; j < RPT; ++j)
      if (pf[j].n >= 0) prefetch(pf[j], pf[j].n);
  } else {
    for (int i = tid; i < R; i += NT) {
      int c;
      pick(i, load(i), c);
    }
  }
  __syncthreads();
  GF_COV_STAMP(1);

  if (greedy && a.mt_key && counter[1] > 0) {
    // COV_GREEDY_RNG: u_ind[i] = np_random.choice(4) for each fallback robot in robot
    // order (:861-864): the k-th fallback robot takes output pos + k of its env's stream.
    // The key goes through LDS; when pos + k passes 624 the key is regenerated in LDS
    // (the earlier words read first) and written back. R <= 624 (checked by the host):
    // at most one regeneration per step.
    uint32_t* kb = reinterpret_cast<uint32_t*>(ucount + 1);
    uint32_t* pm = kb + kMtN;  // fallback robots as bits, 32 per word
    uint32_t* key = a.mt_key + (size_t)b * kMtN;
    const int nfall = counter[1];
    const int pos = a.mt_pos[b];
    {
      const int lane = tid & 63, wv = tid >> 6;
      for (int k0 = wv * 64; k0 < R; k0 += NT) {
        const uint64_t m = __ballot(k0 + lane < R && chosen[k0 + lane] < 0);
        if (lane == 0) {
          pm[k0 >> 5] = static_cast<uint32_t>(m);
          pm[(k0 >> 5) + 1] = static_cast<uint32_t>(m >> 32);
        }
      }
    }
    __syncthreads();
    auto word = [&](int i) {  // the stream index of robot i's draw
      int r = __popc(pm[i >> 5] & ((1u << (i & 31)) - 1u));
      for (int w = 0; w < (i >> 5); ++w) r += __popc(pm[w]);
      return pos + r;
    };
    // the raw words parked in new_s, which the claim resolution below writes first
    for (int i = tid; i < R; i += NT)
      if (chosen[i] < 0 && word(i) < kMtN) new_s[i] = static_cast<int>(kb[word(i)]);
    if (pos + nfall > kMtN) {
      mt_regen<NT>(kb);  // its first barrier orders the reads above before its writes
      for (int i = tid; i < R; i += NT)
        if (chosen[i] < 0 && word(i) >= kMtN) new_s[i] = static_cast<int>(kb[word(i) - kMtN]);
      for (int k = tid; k < kMtN; k += NT) key[k] = kb[k];
    }
    if (tid == 0) a.mt_pos[b] = pos + nfall > kMtN ? pos + nfall - kMtN : pos + nfall;
    auto draw = [&](int i, const int4& offer, Pf* p) {
      const int c = cur_s[i];
      const int ai = static_cast<int>(mt_temper(static_cast<uint32_t>(new_s[i])) & 3u);
      a.gactions[(size_t)b * R + i] = ai;
      const int n = aim(c, ai, offer);
      chosen[i] = n;
      if (n == c) atomicOr(&claim[n >> 5], 1u << (n & 31));
      else if (p) prefetch(*p, n);
    };
    if (one) {
#pragma unroll
      for (int j = 0; j < RPT; ++j) {
        const int i = tid + j * NT;
        if (i < R && chosen[i] < 0) draw(i, ld[j].offer, &pf[j]);
      }
    } else {
      for (int i = tid; i < R; i += NT)
        if (chosen[i] < 0) draw(i, load(i).offer, nullptr);
    }
    __syncthreads();
  }

  if (has_act) {
    // then, in robot order, a move succeeds unless its node is already claimed; a
    // blocked robot stays and its node joins the claims. The reference walks the robots
    // serially; here every robot's outcome is re-evaluated in parallel from the current
    // guesses (the first claimer of each node by atomicMin) until nothing changes. A
    // robot's outcome depends only on lower-indexed robots, so after k rounds robots
    // 0..k-1 are final, and the fixed point is the serial walk's unique result.
    if (R <= 4 * 64) {
      // One wave, up to 4 robots per lane kept in registers; only first[] is in LDS.
      // A wave's LDS operations complete in order, so a round needs no workgroup
      // barrier, only waits for its own LDS operations.
      if (tid < 64) {
        // a wave's LDS instructions execute in issue order, so only the compiler must
        // keep them in order (the reads' results are waited for as used; a fence would
        // also wait for the node prefetch still in flight from global memory)
        auto lds_fence = [] { asm volatile("" ::: "memory"); };
        // four named robots, not an array: an array indexed in a loop stays in scratch
        struct Rb {
          int i, c, n, v;
          bool mv, fr;
        };
        auto init = [&](Rb& r, int i) {
          r.i = i;
          const bool valid = i < R;
          r.c = valid ? cur_s[i] : 0;
          r.n = valid ? chosen[i] : 0;
          r.mv = valid && r.n != r.c;
          r.fr = r.mv && !(claim[r.n >> 5] & (1u << (r.n & 31)));  // not a stayer's node
          r.v = r.n;  // guess: every move succeeds
        };
        // branch-free rounds: a robot that does not move adds INT_MAX (no-op).
        // A mover's claim sits on its chosen node or its own; both are cleared between
        // rounds (a non-mover's own node: no mover's test reads it, since movers onto it
        // are blocked by its stay claim; robots past R sit on node 0, a slot no target uses)
        auto put = [&](const Rb& r) { atomicMin(&first[r.v], r.mv ? r.i : INT_MAX); };
        auto clear = [&](const Rb& r) {
          first[r.n] = INT_MAX;
          first[r.c] = INT_MAX;
        };
        auto eval = [&](Rb& r, int f) {
          const int v = (r.fr && f >= r.i) ? r.n : r.c;  // r.fr implies r.mv
          const bool ch = v != r.v;
          r.v = v;
          return ch;
        };
        Rb r0, r1, r2, r3;
        init(r0, tid);
        init(r1, tid + 64);
        init(r2, tid + 128);
        init(r3, tid + 192);
        while (true) {
          put(r0), put(r1), put(r2), put(r3);
          lds_fence();
          const int f0 = first[r0.n], f1 = first[r1.n], f2 = first[r2.n], f3 = first[r3.n];
          // all four evaluated (no short circuit)
          const int changed = int(eval(r0, f0)) | int(eval(r1, f1)) | int(eval(r2, f2)) | int(eval(r3, f3));
          if (!__any(changed)) break;
          lds_fence();
          clear(r0), clear(r1), clear(r2), clear(r3);
          lds_fence();
        }
        if (r0.i < R) new_s[r0.i] = r0.v;
        if (r1.i < R) new_s[r1.i] = r1.v;
        if (r2.i < R) new_s[r2.i] = r2.v;
        if (r3.i < R) new_s[r3.i] = r3.v;
      }
      __syncthreads();
      GF_COV_STAMP(2);
    } else {
      for (int i = tid; i < R; i += NT) new_s[i] = chosen[i];  // guess: every move succeeds
      while (true) {
        __syncthreads();
        for (int i = tid; i < R; i += NT)
          if (chosen[i] != cur_s[i]) atomicMin(&first[new_s[i]], i);
        __syncthreads();
        int changed = 0;
        for (int i = tid; i < R; i += NT) {
          const int c = cur_s[i], n = chosen[i];
          if (n == c) continue;
          const bool ok = !(claim[n >> 5] & (1u << (n & 31))) && first[n] >= i;
          const int v = ok ? n : c;
          if (v != new_s[i]) {
            new_s[i] = v;
            changed = 1;
          }
        }
        if (!__syncthreads_or(changed)) break;
        for (int i = tid; i < R; i += NT)
          if (chosen[i] != cur_s[i]) {
            first[chosen[i]] = INT_MAX;
            first[cur_s[i]] = INT_MAX;
          }
      }
    }
  } else {
    for (int i = tid; i < R; i += NT) new_s[i] = cur_s[i];
    __syncthreads();
  }

  // move (:198), visit (:265-266, :359) and the observation tail (:259-323)
  float* nodes = a.nodes + (size_t)b * M * 3;
  auto finish = [&](int i, const Pf* p) {
    const int n = new_s[i];
    const int t = n - R;
    const bool moved = n != cur_s[i];
    if (!moved && !full) return;  // same node, same position: its edges stand
    cur[i] = n;
    uint8_t was;
    int4 q;
    float4 d;
    if (moved) {  // on its node's position: the node's record holds its edges
      float4 r0, r1, r2;
      if (p && n == p->n) {
        r0 = p->r0, r1 = p->r1, r2 = p->r2, was = p->was;
      } else {  // R > kCovThreads
        r0 = rec[4 * t], r1 = rec[4 * t + 1], r2 = rec[4 * t + 2], was = vis[t];
      }
      q = make_int4(__float_as_int(r0.x), __float_as_int(r0.y), __float_as_int(r0.z), __float_as_int(r0.w));
      d = r1;
      *reinterpret_cast<float4*>(xr + 2 * i) = r2;
      if constexpr (HID) *reinterpret_cast<float4*>(xr_lds + i) = r2;
    } else {  // a robot that does not move keeps its position (:198)
      int4 q4;
      int nc;
      double2 c0, c1, c2, c3;
      load_node(t, was, q4, nc, c0, c1, c2, c3);
      const double px = xr[2 * i], py = xr[2 * i + 1];
      q = make_int4(0 < nc ? q4.x + R : n, 1 < nc ? q4.y + R : n, 2 < nc ? q4.z + R : n, 3 < nc ? q4.w + R : n);
      d = make_float4(static_cast<float>(dist2d(px, py, c0.x, c0.y) / a.res),
                      static_cast<float>(dist2d(px, py, c1.x, c1.y) / a.res),
                      static_cast<float>(dist2d(px, py, c2.x, c2.y) / a.res),
                      static_cast<float>(dist2d(px, py, c3.x, c3.y) / a.res));
    }
    if (!was) {
      const unsigned old = atomicOr(&seen[n >> 5], 1u << (n & 31));
      if (!(old & (1u << (n & 31)))) {
        vis[t] = 1;
        nodes[3 * n + 2] = 0.0f;
        atomicAdd(counter, 1);
      }
    }
    // the robot's 4 action edges in both directions: six 16-byte stores (base and 4i are
    // multiples of 4 elements, so every group is 16-byte aligned)
    // (the robot's own index never changes: written by full passes only, so a step leaves
    // fewer dirty lines for the end-of-kernel L2 writeback)
    const int k = base + 4 * i;
    *reinterpret_cast<int4*>(snd + k) = q;
    *reinterpret_cast<int4*>(rcv + k + 4 * R) = q;
    if (full) {
      const int4 ii = make_int4(i, i, i, i);
      *reinterpret_cast<int4*>(snd + k + 4 * R) = ii;
      *reinterpret_cast<int4*>(rcv + k) = ii;
    }
    *reinterpret_cast<float4*>(edg + k) = d;
    *reinterpret_cast<float4*>(edg + k + 4 * R) = d;
  };
  if (one) {
#pragma unroll
    for (int j = 0; j < RPT; ++j)
      if (tid + j * NT < R) finish(tid + j * NT, &pf[j]);
  } else {
    for (int i = tid; i < R; i += NT) finish(i, nullptr);
  }
  GF_COV_STAMP(3);
  __syncthreads();
  const int newly = *counter;
  const int nv = nv0 + newly;
  if (tid == 0) {
    a.nvisited[b] = nv;
    a.obs_step[b] = sc0;
    a.step_counter[b] = sc0 + 1;
    a.reward[b] = static_cast<double>(newly);
    a.done[b] = (sc0 + 1 == a.episode_length || nv == T) ? 1 : 0;
    a.dirty[b] = 0;
    if (MULTI && reward_k) reward_k[(size_t)it * a.B + b] = static_cast<double>(newly);
    if (MULTI && done_k) done_k[(size_t)it * a.B + b] = (sc0 + 1 == a.episode_length || nv == T) ? 1 : 0;
  }
  if (a.next_greedy) {
    // controller(greedy=True) (:800-872) on the resulting state, for the next step of an
    // expert loop: this step's visits (the `seen` node bits) joined to the visited bits,
    // then each robot's first unmasked entry of its new node's greedy list
    for (int t = tid; t < T; t += NT) {
      const int n = t + R;
      if ((seen[n >> 5] >> (n & 31)) & 1u) atomicOr(&gvis[t >> 5], 1u << (t & 31));
    }
    __syncthreads();
    const bool ndirect = T - nv <= kGreedyDirectMax;
    if (ndirect) {
      greedy_direct_list(gvis, T, nv > 0, ulist, ucount);
      __syncthreads();
    }
    for (int i = tid; i < R; i += NT) {
      const int c = new_s[i];
      const size_t row = (size_t)b * Tm + (c - R);
      const int g = ndirect ? greedy_direct(a.gcost + row * Tm, a.gprev + row * Tm, nbr + 4 * (c - R), cnt[c - R],
                                            ulist, *ucount)
                            : greedy_from_list(a.glist + row * a.gstride, a.glen + row, gvis, nv > 0, nv >= T);
      const uint32_t flag = static_cast<uint32_t>(g) >> 2;
      if (flag & kGreedyErr) atomicOr(a.err, 8);
      const int ai = (flag & kGreedyRnd) ? 0 : (g & 3);
      const uint8_t nr = (flag & kGreedyRnd) ? 1 : 0;
      a.gactions[(size_t)b * R + i] = ai;
      a.needs_random[(size_t)b * R + i] = nr;
      if (a.h_next) a.h_next[(size_t)b * R + i] = ai;
      if (a.h_nrand) a.h_nrand[(size_t)b * R + i] = nr;
    }
  }
  if (a.h_nodes || a.h_edges || a.h_senders || a.h_receivers || a.h_closest || a.h_step || a.h_err) {
    // cov_step_host: the env's whole observation and step outputs to page-locked host
    // memory, 16-byte stores where both sides are aligned. The workgroup reads back what
    // its own waves wrote above: after the barrier those stores are visible to it.
    __syncthreads();
    auto put = [&](auto* dst, const auto* src, size_t n) {
      using T1 = typename std::remove_const<typename std::remove_pointer<decltype(src)>::type>::type;
      static_assert(sizeof(T1) == 4, "4-byte elements");
      if (!dst) return;
      if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0) {
        const size_t n4 = n >> 2;
        for (size_t k = tid; k < n4; k += NT) reinterpret_cast<int4*>(dst)[k] = reinterpret_cast<const int4*>(src)[k];
        for (size_t k = (n4 << 2) + tid; k < n; k += NT) dst[k] = src[k];
      } else {
        for (size_t k = tid; k < n; k += NT) dst[k] = src[k];
      }
    };
    put(a.h_nodes ? a.h_nodes + (size_t)b * M * 3 : nullptr, nodes, (size_t)M * 3);
    put(a.h_edges ? a.h_edges + (size_t)b * E : nullptr, edg, (size_t)E);
    put(a.h_senders ? a.h_senders + (size_t)b * E : nullptr, snd, (size_t)E);
    put(a.h_receivers ? a.h_receivers + (size_t)b * E : nullptr, rcv, (size_t)E);
    if (a.h_closest)
      for (int i = tid; i < R; i += NT) a.h_closest[(size_t)b * R + i] = new_s[i];
    if (tid == 0) {
      if (a.h_step) a.h_step[b] = sc0;
      if (a.h_reward) a.h_reward[b] = static_cast<double>(newly);
      if (a.h_done) a.h_done[b] = (sc0 + 1 == a.episode_length || nv == T) ? 1 : 0;
      if (a.h_err) a.h_err[b] = __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// Element k of an env's FlattenDictWrapper row (cov_flat_obs_kernel below has the layout)
template <class V>
__device__ __forceinline__ V cov_flat_value(size_t k, size_t M, size_t N, const float* nodes, const float* edges,
                                            const int32_t* snd, const int32_t* rcv, const int64_t* step) {
  if (k < N) return static_cast<V>(nodes[k]);
  if (k < N + 4 * M) return static_cast<V>(edges[k - N]);
  if (k < N + 8 * M) return static_cast<V>(snd[k - N - 4 * M]);
  if (k < N + 12 * M) return static_cast<V>(rcv[k - N - 8 * M]);
  return static_cast<V>(*step);
}

// reset (:405-424 after the random draws) of env b by its workgroup of kCovThreads: robots
// onto their start targets, the unvisited flags, the third node feature, the env's words.
// The observation pass (cov_step_body without actions) follows, after a barrier. count: one
// LDS word. Every thread of the workgroup calls it.
__device__ __forceinline__ void cov_reset_pass(const CovArgs& a, const int b, const int32_t* start,
                                               const uint8_t* visited0, int* count) {
  const int R = a.R, M = a.M, Tm = a.Tmax;
  const int T = a.ntg[b];
  const double* tg = a.tgt + (size_t)b * Tm * 2;
  if (threadIdx.x == 0) *count = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < R; i += kCovThreads) {
    const int t = start[(size_t)b * R + i];
    a.cur[(size_t)b * R + i] = t + R;
    a.xr[((size_t)b * R + i) * 2] = tg[2 * t];
    a.xr[((size_t)b * R + i) * 2 + 1] = tg[2 * t + 1];
  }
  float* nodes = a.nodes + (size_t)b * M * 3;
  int local = 0;
  for (int t = threadIdx.x; t < Tm; t += kCovThreads) {
    const uint8_t v = t < T ? (visited0[(size_t)b * Tm + t] ? 1 : 0) : 1;  // flags are 0 / 1
    a.visited[(size_t)b * Tm + t] = v;
    if (t < T) {
      nodes[3 * (t + R) + 2] = v ? 0.0f : 1.0f;
      local += v ? 1 : 0;
    }
  }
  atomicAdd(count, local);
  __syncthreads();
  if (threadIdx.x == 0) {
    a.nvisited[b] = *count;
    a.step_counter[b] = 0;
    a.dirty[b] = 0;
  }
}

}  // namespace gf
