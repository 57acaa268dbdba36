// reset() of FlockingRelative / Flocking-v0 on the device (flocking_relative.py:156-192):
// each selected env's rejection sampler runs inside one launch, drawing from the env's own
// MT19937 stream (numpy's legacy RandomState, mt19937.h) in the reference's order.
#include <math.h>

#include "flock_internal.h"
#include "mt19937.h"

namespace gf {

namespace {

constexpr int kResetThreads = 256;
constexpr uint8_t kResetExhausted = 1;  // FE_RESET_EXHAUSTED (gymflock.h)
// LDS after the rejection mode's arrays: the key, then bias[2], the smallest a_ij's bits,
// the smallest degree (16-byte multiples throughout)
constexpr size_t kResetMiscBytes = 32;

// np.random.uniform(lo, hi) from random_sample's u: lo + (hi - lo) * u, two roundings
// (the library is compiled with -ffp-contract=off).
__device__ __forceinline__ double uniform_of(double lo, double hi, double u) { return lo + (hi - lo) * u; }

// One workgroup per selected env. A try consumes 4N+2 doubles (8N+4 words) of the stream:
// length[N], angle[N], bias[2], vx[N], vy[N] (:167-174), whether it is accepted or not.
// REJECT: the candidate lives in LDS (positions pl, velocities vl) until one is accepted
// (:176-184) or max_tries are spent (the last one is kept, status FE_RESET_EXHAUSTED);
// else the first candidate is written straight to the state buffer (any N).
// LDS (dynamic, 16-byte parts): pl (N double2), vl (N double2), key (624 words), bias[2],
// min a_ij bits, min degree, deg (N int32); pl, vl and deg only with REJECT.
template <bool REJECT>
__global__ __launch_bounds__(kResetThreads) void flock_reset_kernel(ResetArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NT = kResetThreads;
  const int e = blockIdx.x;
  if (e >= a.n_sel) return;
  const int b = a.envs ? a.envs[e] : e;
  const int tid = threadIdx.x, N = a.N;
  double2* pl = reinterpret_cast<double2*>(smem);
  double2* vl = pl + (REJECT ? N : 0);
  uint32_t* key = reinterpret_cast<uint32_t*>(vl + (REJECT ? N : 0));
  double* bias = reinterpret_cast<double*>(key + kMtN);
  unsigned long long* minbits = reinterpret_cast<unsigned long long*>(bias + 2);
  int* mindeg = reinterpret_cast<int*>(minbits + 1);
  int* deg = mindeg + 2;
  double* xg = a.x + (size_t)b * N * 4;
  // agent i's position and velocity pair of the candidate being drawn
  auto P = [&](int i) -> double* { return REJECT ? reinterpret_cast<double*>(pl + i) : xg + 4 * (size_t)i; };
  auto V = [&](int i) -> double* { return REJECT ? reinterpret_cast<double*>(vl + i) : xg + 4 * (size_t)i + 2; };

  int pos = kMtN;
  if (a.seeded) {
    if (tid == 0) {  // RandomState(seed0 + b): init_genrand
      uint32_t s = a.seed0 + static_cast<uint32_t>(b);
      for (int p = 0; p < kMtN; ++p) {
        key[p] = s;
        s = 1812433253u * (s ^ (s >> 30)) + static_cast<uint32_t>(p + 1);
      }
    }
  } else {
    for (int k = tid; k < kMtN; k += NT) key[k] = a.mt_key[(size_t)b * kMtN + k];
    pos = __builtin_amdgcn_readfirstlane(a.mt_pos[b]);
  }
  __syncthreads();

  // double d of a try from its two stream words, to its place (positions hold length and
  // angle, velocities lack the bias until the try's last word is drawn)
  auto emit = [&](int d, uint32_t wa, uint32_t wb) {
    const double u = (static_cast<double>(wa >> 5) * 67108864.0 + static_cast<double>(wb >> 6)) / 9007199254740992.0;
    if (d < N) {
      P(d)[0] = sqrt(uniform_of(0.0, a.r_max, u));
    } else if (d < 2 * N) {
      P(d - N)[1] = M_PI * uniform_of(0.0, 2.0, u);
    } else if (d < 2 * N + 2) {
      bias[d - 2 * N] = uniform_of(-a.v_bias, a.v_bias, u);
    } else if (d < 3 * N + 2) {
      V(d - 2 * N - 2)[0] = uniform_of(-a.v_max, a.v_max, u);
    } else {
      V(d - 3 * N - 2)[1] = uniform_of(-a.v_max, a.v_max, u);
    }
  };

  const int W = 8 * N + 4;  // words per try
  const int limit = REJECT ? a.max_tries : 1;
  const int G = N < NT ? NT / N : 1;  // pair test: thread groups sharing the columns of a row
  int tries = 0;
  bool ok = false;
  while (tries < limit) {
    // the try's words, key block by key block: words [done, done + take) of the try are
    // key[pos ...]; a double whose words lie either side of a regeneration carries its
    // first word over it
    int done = 0;
    uint32_t carry = 0;
    while (done < W) {
      if (pos == kMtN) {
        mt_regen<NT>(key);  // its first barrier orders the reads below before its writes
        pos = 0;
      }
      const int take = min(kMtN - pos, W - done);
      const int off = pos - done;  // word k of the try is key[off + k]
      if ((done & 1) && tid == 0) emit(done >> 1, carry, mt_temper(key[pos]));
      const int dend = (done + take) >> 1;
      for (int d = ((done + 1) >> 1) + tid; d < dend; d += NT)
        emit(d, mt_temper(key[off + 2 * d]), mt_temper(key[off + 2 * d + 1]));
      if ((done + take) & 1) carry = mt_temper(key[pos + take - 1]);
      done += take;
      pos += take;
    }
    ++tries;
    __syncthreads();
    for (int i = tid; i < N; i += NT) {
      double* p = P(i);
      double* v = V(i);
      const double len = p[0], ang = p[1];
      p[0] = len * cos(ang);
      p[1] = len * sin(ang);
      v[0] += bias[0];
      v[1] += bias[1];
      if (REJECT) deg[i] = 0;
    }
    if (!REJECT) {
      ok = true;
      break;
    }
    if (tid == 0) {
      *minbits = static_cast<unsigned long long>(__double_as_longlong(INFINITY));
      *mindeg = 0x7fffffff;
    }
    __syncthreads();
    // :177-184: a_ij = dx*dx + dy*dy over i != j, its minimum and each row's count below
    // comm_radius^2. a_ij >= 0, so the doubles order as their bit patterns.
    double m = INFINITY;
    for (int r = tid; r < N * G; r += NT) {
      const int g = r / N, i = r - g * N;
      const int j0 = g * N / G, j1 = (g + 1) * N / G;
      const double2 pi = pl[i];
      int c = 0;
#pragma unroll 8
      for (int j = j0; j < j1; ++j) {  // unrolled: the columns' LDS reads go out together
        const double2 pj = pl[j];
        const double dx = pi.x - pj.x, dy = pi.y - pj.y;
        // :179 fill_diagonal(inf) as an exact addition (a_ij >= +0), so no read waits on a branch
        const double aij = (dx * dx + dy * dy) + (j != i ? 0.0 : INFINITY);
        m = fmin(m, aij);
        c += aij < a.cr2 ? 1 : 0;
      }
      atomicAdd(&deg[i], c);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmin(m, __shfl_xor(m, d, 64));
    if ((tid & 63) == 0) atomicMin(minbits, static_cast<unsigned long long>(__double_as_longlong(m)));
    __syncthreads();
    int md = 0x7fffffff;
    for (int i = tid; i < N; i += NT) md = min(md, deg[i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) md = min(md, __shfl_xor(md, d, 64));
    if ((tid & 63) == 0) atomicMin(mindeg, md);
    __syncthreads();
    // every thread reads the same two words: the decision is uniform
    const double min_dist = sqrt(__longlong_as_double(static_cast<long long>(*minbits)));
    const bool reject = *mindeg < a.min_degree || min_dist < a.min_dist;  // :164
    if (!__builtin_amdgcn_readfirstlane(reject ? 1 : 0)) {
      ok = true;
      break;
    }
  }
  if (REJECT) {
    double2* xo = reinterpret_cast<double2*>(xg);
    for (int i = tid; i < N; i += NT) {
      xo[2 * i] = pl[i];
      xo[2 * i + 1] = vl[i];
    }
  }
  for (int k = tid; k < kMtN; k += NT) a.mt_key[(size_t)b * kMtN + k] = key[k];
  if (tid == 0) {
    a.mt_pos[b] = pos;
    a.tries[b] = tries;
    a.status[b] = ok ? 0 : kResetExhausted;
    if (a.seeded) {  // a fresh RandomState has no cached Gaussian (flock_dt_noise.hip)
      a.has_gauss[b] = 0;
      a.gauss[b] = 0.0;
    }
  }
}

}  // namespace

size_t reset_lds_bytes(int N, bool reject) {
  const size_t n = reject ? (size_t)N : 0;
  return n * 32 + (size_t)kMtN * 4 + kResetMiscBytes + (n * 4 + 15) / 16 * 16;
}

hipError_t launch_reset(const ResetArgs& a, hipStream_t s) {
  if (a.n_sel <= 0) return hipSuccess;
  const size_t lds = reset_lds_bytes(a.N, a.reject != 0);
  if (a.reject)
    hipLaunchKernelGGL(flock_reset_kernel<true>, dim3(a.n_sel), dim3(kResetThreads), lds, s, a);
  else
    hipLaunchKernelGGL(flock_reset_kernel<false>, dim3(a.n_sel), dim3(kResetThreads), lds, s, a);
  return hipGetLastError();
}

}  // namespace gf
