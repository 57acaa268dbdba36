// The RCCL metrics path of the flocking C-ABI (fe_comm_*, fe_allgather_*, fe_get_gathered_*):
// the communicator and its worker thread, the side stream with its completion words, the
// bounded host waits and the debug gate. Its state is fe_handle::met (flock_handle.h).
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>

#include "flock_handle.h"

using namespace gf;  // capi_common.h's helpers and flock_handle.h's internal calls

namespace {

// ---- the process's communicator worker
// ncclCommAbort runs on one thread per process that lives until the process exits (never
// on a short-lived thread: RCCL's own threads may keep using the HIP thread-local state of
// the thread that called into it, and a thread that exited under them corrupted the heap
// once torch's HIP runtime was bound). The worker and its queue are never
// destroyed, so the thread outlives static destruction.
struct CommWorker {
  std::mutex mu;
  std::condition_variable cv;
  std::deque<std::pair<ncclComm_t, int>> q;  // (communicator, device)
};

CommWorker* comm_worker() {
  static CommWorker* w = [] {
    auto* p = new CommWorker();
    std::thread([p] {
      for (;;) {
        std::pair<ncclComm_t, int> job;
        {
          std::unique_lock<std::mutex> l(p->mu);
          p->cv.wait(l, [p] { return !p->q.empty(); });
          job = p->q.front();
          p->q.pop_front();
        }
        hipSetDevice(job.second);
        ncclCommAbort(job.first);
      }
    }).detach();
    return p;
  }();
  return w;
}

void abort_comm_later(ncclComm_t c, int device) {
  CommWorker* w = comm_worker();
  {
    std::lock_guard<std::mutex> l(w->mu);
    w->q.emplace_back(c, device);
  }
  w->cv.notify_one();
}

// A thread that called into RCCL's initialisation parks here for the rest of the process
// instead of exiting (the same thread-local-state reason as the worker above).
[[noreturn]] void park_thread() {
  static std::mutex* m = new std::mutex();
  static std::condition_variable* cv = new std::condition_variable();
  std::unique_lock<std::mutex> l(*m);
  for (;;) cv->wait(l);
}

using Clock = std::chrono::steady_clock;

Clock::time_point deadline_in(double seconds) {
  return Clock::now() + std::chrono::microseconds(static_cast<int64_t>(seconds * 1e6));
}

// completion words of the side stream (fe_handle::met.stage_done)
enum { kWordRing = 0, kWordStatsCopy = 1, kWordRewardGather = 2, kWordStatsGather = 3 };

// Whether the side-stream work numbered `seq` on completion word `word` is done (each
// word's kernels run in order on the side stream, so the word only grows).
bool stage_complete(const fe_handle* h, int word, uint32_t seq) {
  return static_cast<int32_t>(__atomic_load_n(h->met.stage_done + word, __ATOMIC_ACQUIRE) - seq) >= 0;
}

int no_comm(const fe_handle* h) {
  return fail(GF_ESTATE, "no communicator (fe_comm_init not called, or it was torn down" +
                             (h->met.comm_lost.empty() ? std::string(")") : ": " + h->met.comm_lost + ")"));
}

// A non-blocking communicator's pending work: poll its async error until it leaves
// ncclInProgress or the deadline passes; then the metrics path is torn down (the
// communicator aborted), so no rank waits forever on a peer that never joined or died.
int comm_wait(fe_handle* h, Clock::time_point deadline, const char* what) {
  for (;;) {
    ncclResult_t st = ncclSuccess;
    ncclResult_t r = ncclCommGetAsyncError(h->met.comm, &st);
    if (r != ncclSuccess) st = r;
    if (st == ncclSuccess) return GF_OK;
    if (st != ncclInProgress || Clock::now() > deadline) {
      comm_release(h, true);
      h->met.comm_lost = std::string(what) + ": " +
                         (st != ncclInProgress ? std::string(ncclGetErrorString(st))
                                               : std::string("timed out (a rank did not join or stopped responding)")) +
                         "; communicator aborted";
      return fail(GF_ECOMM, h->met.comm_lost);
    }
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
}

// Wait for side-stream work `seq` on completion word `word` (a gather's staging copy or
// its collective), polling the communicator's async error beside it: on expiry of the
// collective timeout (a rank that died mid-run never posts its part) or a communicator
// error the metrics path is torn down (GF_ECOMM, comm_lost says why); a side stream that
// finished without the word is a HIP error (the path stays up).
int stage_wait(fe_handle* h, int word, uint32_t seq, const char* what) {
  const auto deadline = deadline_in(h->met.comm_timeout);
  for (int spin = 0;; ++spin) {
    h->met.dbg[7] = spin;
    if (stage_complete(h, word, seq)) return GF_OK;
    if ((spin & 63) == 63) {
      const hipError_t q = hipStreamQuery(h->met.comm_stream);
      if (q == hipSuccess && !stage_complete(h, word, seq))
        return fail(GF_EHIP, std::string(what) + ": the side stream finished without the copy's completion word");
      if (q != hipSuccess && q != hipErrorNotReady) return fail_hip(what, q);
    }
    ncclResult_t st = ncclSuccess;
    ncclResult_t r = ncclCommGetAsyncError(h->met.comm, &st);
    if (r != ncclSuccess) st = r;
    if (spin == 0) h->met.dbg[3] = static_cast<int32_t>(st);
    const bool err = st != ncclSuccess && st != ncclInProgress;
    if (err || Clock::now() > deadline) {
      comm_release(h, true);
      h->met.comm_lost = std::string(what) + ": " +
                         (err ? std::string(ncclGetErrorString(st)) : std::string("timed out (a rank stopped responding)")) +
                         "; communicator aborted";
      return fail(GF_ECOMM, h->met.comm_lost);
    }
    if (spin > 64) std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
}

// A collective just enqueued on the non-blocking communicator: wait until it is queued.
int comm_enqueued(fe_handle* h, ncclResult_t r, const char* what) {
  if (r == ncclInProgress) return comm_wait(h, deadline_in(h->met.comm_timeout), what);
  if (r != ncclSuccess) {
    comm_release(h, true);
    h->met.comm_lost = std::string(what) + ": " + ncclGetErrorString(r) + "; communicator aborted";
    return fail(GF_ECOMM, h->met.comm_lost);
  }
  return GF_OK;
}

// A zeroed device buffer of the metrics path (the pad columns of the send blocks are
// never written afterwards).
template <class T>
int comm_alloc(fe_handle* h, T** p, size_t count) {
  if (int rc = dalloc(p, count)) return rc;
  if (*p) GF_HIP(hipMemsetAsync(*p, 0, count * sizeof(T), h->met.comm_stream));
  return GF_OK;
}

// fe_comm_init once the communicator exists: the side stream, the shard-size exchange
// and the gather buffers. On failure the caller tears everything down.
int comm_setup(fe_handle* h, int nranks, int rank, Clock::time_point deadline) {
  auto& m = h->met;
  GF_HIP(hipStreamCreateWithFlags(&m.comm_stream, hipStreamNonBlocking));
  if (!m.stage_done) {
    void* p = nullptr;
    GF_HIP(hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocCoherent));
    m.stage_done = static_cast<uint32_t*>(p);
    for (int w = 0; w < 4; ++w)  // every earlier sequence number: done
      __atomic_store_n(m.stage_done + w, m.stage_seq[w], __ATOMIC_SEQ_CST);
    void* d = nullptr;
    GF_HIP(hipHostGetDevicePointer(&d, p, 0));
    m.stage_done_dev = static_cast<uint32_t*>(d);
  }
  // every rank's shard size, before any gather pads to the largest
  int32_t* dsz = nullptr;
  if (int rc = dalloc(&dsz, (size_t)nranks)) return rc;
  std::vector<int32_t> sizes(nranks);
  const int32_t mine = h->cfg.n_envs;
  int rc = GF_OK;
  const hipError_t e = hipMemcpyAsync(dsz + rank, &mine, 4, hipMemcpyHostToDevice, m.comm_stream);
  if (e != hipSuccess) rc = fail_hip("shard-size upload", e);
  if (rc == GF_OK) {
    const ncclResult_t r = ncclAllGather(dsz + rank, dsz, 1, ncclInt32, m.comm, m.comm_stream);
    rc = (r == ncclSuccess || r == ncclInProgress) ? comm_wait(h, deadline, "shard-size all-gather")
                                                   : fail(GF_ECOMM, std::string("ncclAllGather: ") + ncclGetErrorString(r));
  }
  if (rc == GF_OK) {
    hipError_t q;
    while ((q = hipStreamQuery(m.comm_stream)) == hipErrorNotReady) {
      if (Clock::now() > deadline) break;
      std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    if (q == hipErrorNotReady) {
      rc = fail(GF_ECOMM, "shard-size all-gather: timed out (a rank stopped responding)");
    } else if (q != hipSuccess) {
      rc = fail(GF_EHIP, std::string("shard-size all-gather: ") + hipGetErrorString(q));
    } else if (hipMemcpyAsync(sizes.data(), dsz, 4 * (size_t)nranks, hipMemcpyDeviceToHost, m.comm_stream) !=
                   hipSuccess ||
               hipStreamSynchronize(m.comm_stream) != hipSuccess) {
      rc = fail(GF_EHIP, "shard-size copy");
    } else {
      rc = fe_check_shard_sizes(nranks, sizes.data());
    }
  }
  hipFree(dsz);
  if (rc != GF_OK) return rc;
  m.shard_sizes = sizes;
  m.max_envs = *std::max_element(sizes.begin(), sizes.end());
  const size_t W = m.max_envs;
  for (hipEvent_t* e : {&m.step_ev, &m.step_ev2})
    GF_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  if ((rc = comm_alloc(h, &m.gsend, (size_t)kRewardSlots * W)) ||
      (rc = comm_alloc(h, &m.gather, (size_t)nranks * kRewardSlots * W)) || (rc = comm_alloc(h, &m.ssend, W * 2)) ||
      (rc = comm_alloc(h, &m.stats_gather, (size_t)nranks * W * 2)))
    return rc;
  GF_HIP(hipStreamSynchronize(m.comm_stream));
  m.nranks = nranks;
  m.rank = rank;
  m.gathered_upto = h->steps_written;  // the first gather ships the steps after init
  return GF_OK;
}

}  // namespace

namespace gf {

// Every collective on the side stream complete, polled against the collective timeout and
// the communicator's async error; false when it expired (a peer stopped responding).
bool comm_stream_drained(fe_handle* h) {
  if (!h->met.comm_stream) return true;
  const auto deadline = deadline_in(h->met.comm_timeout);
  for (int spin = 0;; ++spin) {
    const hipError_t q = hipStreamQuery(h->met.comm_stream);
    if (q != hipErrorNotReady) return q == hipSuccess;
    ncclResult_t st = ncclSuccess;
    if (h->met.comm &&
        (ncclCommGetAsyncError(h->met.comm, &st) != ncclSuccess || (st != ncclSuccess && st != ncclInProgress)))
      return false;
    if (Clock::now() > deadline) return false;
    if (spin > 64) std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
}

// Tear down the metrics path: the communicator (aborted when a collective may never
// complete, else destroyed once the side stream has drained) and everything fe_comm_init
// made for it, so that a later fe_comm_init starts from scratch.
//
// abort: a collective (or the initialisation) may never finish because a peer is gone.
// The communicator is then aborted on the process's communicator worker, and the side
// stream, its events and the buffers its collectives use are abandoned rather than
// synchronised or freed (a kernel of the aborted collective may still touch them), so
// that this call cannot hang; the step streams never wait on the side stream. A
// non-abort release whose side stream does not drain within the collective timeout
// becomes an abort.
void comm_release(fe_handle* h, bool abort) {
  auto& m = h->met;
  if (!abort && m.comm && !comm_stream_drained(h)) abort = true;
  if (abort) {
    if (m.comm) abort_comm_later(m.comm, h->cfg.device);
    m.comm = nullptr;
    m.comm_stream = nullptr;
    m.step_ev = m.step_ev2 = nullptr;
    m.ring_reads.clear();  // copies the side stream may still run: abandoned, and so
    m.stage_done = m.stage_done_dev = nullptr;  // is the word they would store into
    m.gsend = m.gather = m.ssend = m.stats_gather = nullptr;
  }
  if (m.comm) {
    ncclCommDestroy(m.comm);
    m.comm = nullptr;
  }
  if (m.comm_stream) {
    hipStreamSynchronize(m.comm_stream);  // drained above
    hipStreamDestroy(m.comm_stream);
    m.comm_stream = nullptr;
  }
  for (hipEvent_t* e : {&m.step_ev, &m.step_ev2})
    if (*e) {
      hipEventDestroy(*e);
      *e = nullptr;
    }
  m.ring_reads.clear();
  for (double** p : {&m.gsend, &m.gather, &m.ssend, &m.stats_gather})
    if (*p) {
      hipFree(*p);
      *p = nullptr;
    }
  m.ag_issued = m.sg_pending = false;
  m.last_count = 0;
  m.nranks = 1;
  m.rank = 0;
  m.max_envs = 0;
  m.shard_sizes.clear();
}

// The reward ring advances before a launch that writes rewards (next_reward_slot, capi.hip).
// The slot last held the step kRewardSlots launches back. A reward gather's staging copy
// (on the side stream, behind the previous collectives) that may still read it has normally
// finished long ago: its completion word is read on the host. If not, the host waits for
// it, bounded by the collective timeout; on expiry (a collective stuck on a peer that
// stopped responding) the metrics path is torn down (the communicator aborted, the reason
// kept in comm_lost for the next metrics call) and the step goes on. The step streams
// never wait on the side stream on the device, so nothing queued behind a stuck collective
// can stall them.
int ring_reads_wait(fe_handle* h, int64_t s) {
  auto& m = h->met;
  while (!m.ring_reads.empty() && m.ring_reads.front().first <= s - kRewardSlots) {
    const uint32_t seq = m.ring_reads.front().seq;
    const bool done = stage_complete(h, kWordRing, seq);
    m.dbg[0]++;
    m.dbg[1] = done ? 1 : 0;
    m.dbg[2] = -1;
    if (!done) {
      m.dbg[2] = stage_wait(h, kWordRing, seq, "reward all-gather staging copy (ring slot reuse)");
      if (m.dbg[2] == GF_ECOMM) break;  // comm_release emptied ring_reads: the step goes on
      if (m.dbg[2] != GF_OK) return m.dbg[2];
    }
    m.ring_reads.pop_front();
  }
  return GF_OK;
}

// A pending stats gather's staging copy may still read stats_sum: the host waits for it
// (bounded, as ring_reads_wait; on expiry the metrics path is torn down and the summary
// goes on).
int stats_send_wait(fe_handle* h) {
  auto& m = h->met;
  if (m.sg_pending && m.comm && !stage_complete(h, kWordStatsCopy, m.stage_seq[kWordStatsCopy])) {
    const int rc = stage_wait(h, kWordStatsCopy, m.stage_seq[kWordStatsCopy], "stats all-gather (send block reuse)");
    if (rc != GF_OK && rc != GF_ECOMM) return rc;  // GF_ECOMM: torn down, the summary goes on
  }
  return GF_OK;
}

}  // namespace gf

extern "C" {

int fe_comm_unique_id(uint8_t id[128]) {
  if (!id) return fail(GF_EINVAL, "null argument");
  ncclUniqueId uid;
  ncclResult_t r = ncclGetUniqueId(&uid);
  if (r != ncclSuccess) return fail(GF_ECOMM, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
  static_assert(sizeof(uid) == 128, "ncclUniqueId size");
  std::memcpy(id, &uid, 128);
  return GF_OK;
}

int fe_check_shard_sizes(int nranks, const int32_t* n_envs) {
  if (nranks < 1 || !n_envs) return fail(GF_EINVAL, "bad argument");
  for (int r = 0; r < nranks; ++r)
    if (n_envs[r] < 1) {
      std::string m = "bad env shard sizes over ranks (every rank holds at least one env): n_envs =";
      for (int q = 0; q < nranks; ++q) m += " " + std::to_string(n_envs[q]);
      return fail(GF_ECOMM, m);
    }
  return GF_OK;
}

int fe_comm_init_timeout(fe_handle* h, int nranks, int rank, const uint8_t id[128], double timeout_s) {
  if (!h || !id || nranks < 1 || rank < 0 || rank >= nranks || !(timeout_s > 0)) return fail(GF_EINVAL, "bad argument");
  if (h->met.comm) return fail(GF_ESTATE, "communicator already initialised");
  if (int rc = use_dev(h)) return rc;
  const auto deadline = deadline_in(timeout_s);
  h->met.comm_timeout = timeout_s;
  ncclUniqueId uid;
  std::memcpy(&uid, id, 128);
  // RCCL's non-blocking init still connects to the bootstrap root inside the call, which
  // waits for every rank: with a rank missing it never returns. The call therefore runs
  // on a thread of its own, which also waits for the communicator to leave
  // ncclInProgress (RCCL's own init thread works on the creating thread's HIP state:
  // with torch's HIP runtime bound, a creating thread that exited first left a corrupted
  // heap) and then parks for the rest of the process instead of exiting. It hands the
  // communicator over through `state`: 0 running, 1 handed over, 2 abandoned by this call
  // at the deadline (the helper then queues what it created for the communicator
  // worker's abort), so exactly one side owns the communicator. This rank then fails
  // with GF_ECOMM, its handle still usable.
  struct InitJob {
    ncclComm_t comm = nullptr;
    ncclResult_t r = ncclInProgress;
    std::atomic<int> state{0};
  };
  auto job = std::make_shared<InitJob>();
  const int dev = h->cfg.device;
  std::thread([job, nranks, uid, rank, dev]() {
    hipSetDevice(dev);
    ncclConfig_t config = NCCL_CONFIG_INITIALIZER;
    config.blocking = 0;
    ncclComm_t c = nullptr;
    ncclResult_t rr = ncclCommInitRankConfig(&c, nranks, uid, rank, &config);
    if (c && (rr == ncclSuccess || rr == ncclInProgress)) {
      for (;;) {
        ncclResult_t st = ncclSuccess;
        const ncclResult_t q = ncclCommGetAsyncError(c, &st);
        rr = q != ncclSuccess ? q : st;
        if (rr != ncclInProgress || job->state.load(std::memory_order_acquire) == 2) break;
        std::this_thread::sleep_for(std::chrono::microseconds(200));
      }
    }
    job->comm = c;
    job->r = rr;
    int running = 0;
    if (!job->state.compare_exchange_strong(running, 1, std::memory_order_acq_rel) && c)
      abort_comm_later(c, dev);  // abandoned: nobody else will release it
    park_thread();
  }).detach();
  while (job->state.load(std::memory_order_acquire) != 1) {
    if (Clock::now() > deadline) {
      int running = 0;
      if (job->state.compare_exchange_strong(running, 2, std::memory_order_acq_rel))
        return fail(GF_ECOMM, "ncclCommInitRankConfig: timed out (a rank did not join); the initialisation is aborted behind");
      break;  // handed over just now
    }
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
  h->met.comm = job->comm;
  h->met.comm_lost.clear();
  const ncclResult_t r = job->r;
  if (r != ncclSuccess && r != ncclInProgress) {
    comm_release(h, true);
    return fail(GF_ECOMM, std::string("ncclCommInitRankConfig: ") + ncclGetErrorString(r));
  }
  if (int rc = comm_wait(h, deadline, "ncclCommInitRankConfig")) return rc;
  if (int rc = comm_setup(h, nranks, rank, deadline)) {
    const std::string msg = fe_last_error();
    comm_release(h, true);  // abort: a peer may still be inside the shard-size collective
    return fail(rc, msg);
  }
  return GF_OK;
}

int fe_comm_init(fe_handle* h, int nranks, int rank, const uint8_t id[128]) {
  return fe_comm_init_timeout(h, nranks, rank, id, kCommInitTimeoutS);
}

int fe_comm_info(fe_handle* h, int32_t* count, int32_t* user_rank, int32_t* device, char* bus_id, int bus_id_len) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->met.comm) return no_comm(h);
  int c = 0, ur = 0, d = 0;
  ncclResult_t r = ncclCommCount(h->met.comm, &c);
  if (r == ncclSuccess) r = ncclCommUserRank(h->met.comm, &ur);
  if (r == ncclSuccess) r = ncclCommCuDevice(h->met.comm, &d);
  if (r != ncclSuccess) return fail(GF_ECOMM, std::string("ncclComm query: ") + ncclGetErrorString(r));
  if (count) *count = c;
  if (user_rank) *user_rank = ur;
  if (device) *device = d;
  if (bus_id && bus_id_len > 0) GF_HIP(hipDeviceGetPCIBusId(bus_id, bus_id_len, d));
  return GF_OK;
}

int fe_comm_shard_sizes(fe_handle* h, int32_t* sizes, int32_t* max_envs) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->met.comm) return no_comm(h);
  if (sizes) std::copy(h->met.shard_sizes.begin(), h->met.shard_sizes.end(), sizes);
  if (max_envs) *max_envs = h->met.max_envs;
  return GF_OK;
}

}  // extern "C"

namespace {
// A reward gather's staging copy on the side stream: steps [s0, s0 + count) of the ring
// (wrapping) into the padded send block, then `seq` into the page-locked completion word
// with a system-scope release once every read of the ring has returned.
__global__ __launch_bounds__(256) void ring_stage_kernel(const double* ring, int B, int s0, int count, double* gs,
                                                         int W, uint32_t* done, uint32_t seq) {
  const int n = count * B;
  for (int k = threadIdx.x; k < n; k += 256) {
    const int t = k / B, e = k - t * B;
    gs[(size_t)t * W + e] = ring[(size_t)((s0 + t) % kRewardSlots) * B + e];
  }
  __syncthreads();  // every thread's loads returned (its stores used them)
  if (threadIdx.x == 0) {
    __threadfence_system();
    __hip_atomic_store(done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// After a collective on the side stream: `seq` into its completion word (the stream's
// earlier work, the collective included, is complete when this runs).
__global__ __launch_bounds__(64) void signal_kernel(uint32_t* done, uint32_t seq) {
  if (threadIdx.x == 0) {
    __threadfence_system();
    __hip_atomic_store(done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// The stats gather's send block: n doubles from the summaries, then `seq` into the
// completion word once every read of them has returned.
__global__ __launch_bounds__(256) void copy_signal_kernel(const double* src, double* dst, int n, uint32_t* done,
                                                          uint32_t seq) {
  for (int k = threadIdx.x; k < n; k += 256) dst[k] = src[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence_system();
    __hip_atomic_store(done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
}  // namespace

extern "C" {

int fe_allgather_rewards(fe_handle* h) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->met.comm) return no_comm(h);
  // a step-path call: the gather's stream waits for both step streams' latest work
  // (events only), so back-to-back split steps around it stay split and out of phase
  // (use_dev's join would make the next step a single launch)
  if (int rc = use_dev_step(h)) return rc;
  auto& m = h->met;
  const int64_t first = m.gathered_upto, count = h->steps_written - first;
  if (count <= 0) return fail(GF_ESTATE, "no step since the last reward all-gather");
  if (count > kRewardSlots) {
    // the ranks step in lockstep, so every rank takes this branch at the same call and
    // none is left inside a collective
    m.gathered_upto = h->steps_written;
    return fail(GF_ESTATE, "the rewards of " + std::to_string(count - kRewardSlots) +
                               " step(s) were overwritten before a gather (gather at least every " +
                               std::to_string(kRewardSlots) + " steps)");
  }
  const size_t B = h->cfg.n_envs, W = m.max_envs;
  // the side stream waits for both step streams' latest work (events only; the step
  // streams never wait for the side stream)
  GF_HIP(hipEventRecord(m.step_ev, h->stream));
  GF_HIP(hipStreamWaitEvent(m.comm_stream, m.step_ev, 0));
  if (h->stream2) {
    GF_HIP(hipEventRecord(m.step_ev2, h->stream2));
    GF_HIP(hipStreamWaitEvent(m.comm_stream, m.step_ev2, 0));
  }
  // the steps' ring slots (two runs when they wrap) into the padded send block, behind
  // the previous collective (which read it) on the same stream
  // and their completion into the page-locked word the ring-slot reuse polls: the copy
  // kernel's own store, not an event query ("a step that did not wait")
  double* gs = m.gsend;
  const int s0 = static_cast<int>(first % kRewardSlots);
  const uint32_t seq = ++m.stage_seq[kWordRing];
  hipLaunchKernelGGL(ring_stage_kernel, dim3(1), dim3(256), 0, m.comm_stream, static_cast<const double*>(h->reward_ring),
                     static_cast<int>(B), s0, static_cast<int>(count), gs, static_cast<int>(W),
                     m.stage_done_dev + kWordRing, seq);
  GF_HIP(hipGetLastError());
  m.ring_reads.push_back({first, seq});
  m.dbg[4] = static_cast<int32_t>(m.ring_reads.size());
  m.dbg[5] = stage_complete(h, kWordRing, seq) ? 1 : 0;
  if (int rc = comm_enqueued(h, ncclAllGather(gs, m.gather, (size_t)count * W, ncclFloat64, m.comm, m.comm_stream),
                             "ncclAllGather (rewards)"))
    return rc;
  hipLaunchKernelGGL(signal_kernel, dim3(1), dim3(64), 0, m.comm_stream, m.stage_done_dev + kWordRewardGather,
                     ++m.stage_seq[kWordRewardGather]);
  GF_HIP(hipGetLastError());
  m.ag_issued = true;
  m.last_count = static_cast<int>(count);
  m.gathered_upto = h->steps_written;
  return GF_OK;
}

int fe_get_gathered_rewards(fe_handle* h, double* dst) {
  if (!h || !dst) return fail(GF_EINVAL, "null argument");
  if (!h->met.comm) return no_comm(h);
  if (!h->met.ag_issued) return fail(GF_ESTATE, "no all-gather issued");
  if (int rc = use_dev(h)) return rc;
  if (int rc = stage_wait(h, kWordRewardGather, h->met.stage_seq[kWordRewardGather], "reward all-gather")) return rc;
  const size_t n = (size_t)h->met.nranks * h->met.last_count * h->met.max_envs;
  return d2h(h, dst, h->met.gather, n * 8);  // (on the handle's stream: no use of the null stream)
}

int fe_gathered_steps(fe_handle* h) { return h ? h->met.last_count : 0; }

int fe_allgather_stats(fe_handle* h) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (!h->met.comm) return no_comm(h);
  if (!h->has_state) return fail(GF_ESTATE, "state not set");
  // the summaries are taken on the whole current state (both step halves joined); the
  // collective then runs on the side stream, like the reward all-gather
  if (int rc = use_dev(h)) return rc;
  if (int rc = stats_summary_dev(h)) return rc;  // (after the previous stats gather, bounded)
  auto& m = h->met;
  if (!m.comm) return fail(GF_ECOMM, "metrics path torn down: " + m.comm_lost);
  GF_HIP(hipEventRecord(m.step_ev, h->stream));
  GF_HIP(hipStreamWaitEvent(m.comm_stream, m.step_ev, 0));
  // into the padded send block, on the side stream (after the previous stats gather)
  hipLaunchKernelGGL(copy_signal_kernel, dim3(1), dim3(256), 0, m.comm_stream, static_cast<const double*>(h->stats_sum),
                     m.ssend, h->cfg.n_envs * 2, m.stage_done_dev + kWordStatsCopy, ++m.stage_seq[kWordStatsCopy]);
  GF_HIP(hipGetLastError());
  if (int rc = comm_enqueued(h, ncclAllGather(m.ssend, m.stats_gather, (size_t)m.max_envs * 2, ncclFloat64, m.comm,
                                              m.comm_stream),
                             "ncclAllGather (stats)"))
    return rc;
  hipLaunchKernelGGL(signal_kernel, dim3(1), dim3(64), 0, m.comm_stream, m.stage_done_dev + kWordStatsGather,
                     ++m.stage_seq[kWordStatsGather]);
  GF_HIP(hipGetLastError());
  m.sg_pending = true;
  return GF_OK;
}

int fe_get_gathered_stats(fe_handle* h, double* dst) {
  if (!h || !dst) return fail(GF_EINVAL, "null argument");
  if (!h->met.comm) return no_comm(h);
  if (!h->met.sg_pending) return fail(GF_ESTATE, "no stats all-gather issued");
  if (int rc = use_dev(h)) return rc;
  if (int rc = stage_wait(h, kWordStatsGather, h->met.stage_seq[kWordStatsGather], "stats all-gather")) return rc;
  return d2h(h, dst, h->met.stats_gather, (size_t)h->met.nranks * h->met.max_envs * 2 * sizeof(double));
}

int fe_comm_destroy(fe_handle* h) {
  if (!h) return fail(GF_EINVAL, "null handle");
  if (int rc = use_dev(h)) return rc;
  comm_release(h, false);
  return GF_OK;
}

}  // extern "C"

namespace {
// fe_debug_comm_gate's kernel: one wave that sleeps until the page-locked flag turns
// non-zero or `ticks` of the device's wall clock pass (always bounded).
// flag[1] = 1 once it runs, flag[2] = 1 (opened) or 2 (timed out) as it ends.
__global__ __launch_bounds__(64) void comm_gate_kernel(unsigned* flag, unsigned long long ticks) {
  const unsigned long long t0 = wall_clock64();
  if (threadIdx.x == 0) __hip_atomic_store(flag + 1, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  unsigned why = 1u;
  while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u) {
    if (wall_clock64() - t0 > ticks) {
      why = 2u;
      break;
    }
    __builtin_amdgcn_s_sleep(127);
  }
  if (threadIdx.x == 0) __hip_atomic_store(flag + 2, why, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// one process-wide gate flag (fine-grained page-locked memory), never freed: a gate
// kernel abandoned with an aborted side stream may still read it
unsigned* gate_flag() {
  static unsigned* f = [] {
    void* p = nullptr;
    if (hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return (unsigned*)nullptr;
    *static_cast<unsigned*>(p) = 1u;
    return static_cast<unsigned*>(p);
  }();
  return f;
}

// the path of the shared object that defines the function at `fn`
void so_path(const void* fn, char* dst, int len) {
  if (!dst || len <= 0) return;
  Dl_info info{};
  const char* p = (dladdr(fn, &info) && info.dli_fname) ? info.dli_fname : "";
  std::snprintf(dst, (size_t)len, "%s", p);
}
}  // namespace

extern "C" {

int fe_debug_comm_gate(fe_handle* h, int close, double max_seconds) {
  if (!h) return fail(GF_EINVAL, "null handle");
  unsigned* f = gate_flag();
  if (!f) return fail(GF_ENOMEM, "gate flag: hipHostMalloc failed");
  if (!close) {  // also after the communicator was aborted (its side stream abandoned)
    __atomic_store_n(f, 1u, __ATOMIC_SEQ_CST);
    return GF_OK;
  }
  if (!h->met.comm || !h->met.comm_stream) return fail(GF_ESTATE, "no communicator (fe_comm_init first)");
  if (!(max_seconds > 0) || max_seconds > 120) return fail(GF_EINVAL, "max_seconds must be in (0, 120]");
  GF_HIP(hipSetDevice(h->cfg.device));
  int khz = 0;
  GF_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->cfg.device));
  void* df = nullptr;
  GF_HIP(hipHostGetDevicePointer(&df, f, 0));
  __atomic_store_n(f + 1, 0u, __ATOMIC_SEQ_CST);
  __atomic_store_n(f + 2, 0u, __ATOMIC_SEQ_CST);
  __atomic_store_n(f, 0u, __ATOMIC_SEQ_CST);
  const unsigned long long ticks = static_cast<unsigned long long>(max_seconds * 1000.0 * (khz > 0 ? khz : 100000));
  hipLaunchKernelGGL(comm_gate_kernel, dim3(1), dim3(64), 0, h->met.comm_stream, static_cast<unsigned*>(df), ticks);
  GF_HIP(hipGetLastError());
  h->met.dbg[6] = static_cast<int32_t>(hipStreamQuery(h->met.comm_stream));
  return GF_OK;
}

int fe_debug_comm_state(fe_handle* h, int32_t* out) {
  if (!h || !out) return fail(GF_EINVAL, "null argument");
  for (int k = 0; k < 8; ++k) out[k] = h->met.dbg[k];
  unsigned* f = gate_flag();
  out[8] = f ? static_cast<int32_t>(__atomic_load_n(f + 1, __ATOMIC_SEQ_CST)) : -1;
  out[9] = f ? static_cast<int32_t>(__atomic_load_n(f + 2, __ATOMIC_SEQ_CST)) : -1;
  out[10] = h->met.comm ? 1 : 0;
  out[11] = static_cast<int32_t>(h->met.ring_reads.size());
  return GF_OK;
}

int fe_runtime_info(int32_t* hip_runtime_version, int32_t* hip_driver_version, int32_t* rccl_version, char* hip_path,
                    int hip_path_len, char* rccl_path, int rccl_path_len) {
  int v = 0;
  if (hip_runtime_version) *hip_runtime_version = hipRuntimeGetVersion(&v) == hipSuccess ? v : 0;
  v = 0;
  if (hip_driver_version) {
    *hip_driver_version = hipDriverGetVersion(&v) == hipSuccess ? v : 0;
    (void)hipGetLastError();
  }
  v = 0;
  if (rccl_version) *rccl_version = ncclGetVersion(&v) == ncclSuccess ? v : 0;
  so_path(reinterpret_cast<const void*>(&hipRuntimeGetVersion), hip_path, hip_path_len);
  so_path(reinterpret_cast<const void*>(&ncclGetVersion), rccl_path, rccl_path_len);
  return GF_OK;
}

}  // extern "C"
