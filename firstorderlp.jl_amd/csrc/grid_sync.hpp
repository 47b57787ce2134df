// grid_sync.hpp -- part of the single translation unit pdhg_hip.hip (included there, before the first kernel that publishes).
// What every persistent (one-launch) kernel here shares, stated once: the XCD-scoped grid barrier, the "last workgroup
// finishes" ticket, and the result words a launch hands to the host through pinned memory (publisher, checksum, waiter).
// These few lines decide whether a launch hangs, times out cleanly or hands the host a torn result.
//
// Grid barrier (measured: tools/grid_barrier_probe.hip, profiles/r03_grid_barrier_probe.txt).
// An agent-scope release / acquire on this chip writes back / invalidates the XCD's L2
// (buffer_wbl2 sc1 / buffer_inv sc1), and when every workgroup issues its own they serialise
// in the L2: 9.4 us per barrier for 256 workgroups, 19 us for 512, 65 us for 2048, whatever
// the counter structure (flat, tree, per-XCD).  So the fences are scoped by hand: a
// workgroup's stores are in its XCD's L2 once `s_waitcnt vmcnt(0)` returns (the L1 is
// write-through); it then arrives on its XCD's counter; only the LAST arriver of the XCD writes
// the L2 back, arrives on the global counter, waits for all 8 XCDs, invalidates the L2 and
// releases its XCD.  3.2 / 3.8 / 5.0 / 7.4 us for 256 / 512 / 1024 / 2048 workgroups.
// The other workgroups do NOT invalidate their CU's L1 (`buffer_inv sc0` is a no-op on this
// chip, `sc1` would serialise in the L2 again): not needed for the trial kernel's data flow -- the
// L1 is clean at kernel start and no address is read before the phase that produces it has
// completed (x', xbar: written in phase 0, read from phase 1 on; y': written in phase 1, read
// in phase 2; partial sums: read at the end only), so no CU can hold a stale line.
// The XCD of a workgroup comes from the hardware register (XCC_ID); how many workgroups of a
// launch land on each XCD is counted once per handle by a registration launch of the same
// shape (the dispatcher deals workgroups round-robin; the probe saw exact, repeatable counts).
// Every spin is bounded: a barrier that cannot complete (workgroups not co-resident because
// the device is shared) raises the error word instead of hanging, and the host reports it.
// The codes: 2 / 3 grid_barrier (leader / waiter), 4 / 5 steps_kernel's third barrier, 6 / 7 / 8 group_barrier.
#pragma once

namespace {

struct GridSync {                           // device memory, one per handle; one 128-byte line per word
  unsigned long long global[16];            // XCD leaders arrived (monotonic over launches)
  unsigned long long xcd_arrive[8][16];
  unsigned long long xcd_release[8][16];    // last completed barrier epoch of the XCD
  unsigned long long xcd_count[8][16];      // workgroups of one launch on each XCD
  unsigned long long xcd_done[8][16];       // workgroups of the XCD that have finished their last phase
  unsigned long long ticket[3][16];         // [2]: XCDs done (the last workgroup of the last XCD runs the second-stage reduction)
  unsigned long long error[16];
  unsigned long long xrelease[16];          // group_kernel.hpp: last cross-shard barrier the shard's last XCD leader has passed
};

__device__ __forceinline__ unsigned xcc_id() {
  return __builtin_amdgcn_s_getreg(((4 - 1) << 11) | (0 << 6) | 20) & 7;   // hwreg(HW_REG_XCC_ID, 0, 4)
}

__global__ __launch_bounds__(TPB) void xcd_register_kernel(GridSync *s) {
  if (threadIdx.x == 0) __hip_atomic_fetch_add(&s->xcd_count[xcc_id()][0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr long GRID_SPIN_LIMIT = 4000000L;   // x s_sleep(1): ~0.1 s

// store that is visible device-wide once `s_waitcnt vmcnt(0)` has returned (write-through,
// no L2 write-back needed): the few words a workgroup hands to a "last one finishes" ticket
__device__ __forceinline__ void store_agent(double *p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the barrier -------------------------------------------------------------------------------------------------
// The skeleton of every barrier here.  Thread 0 of each workgroup, once its workgroup's stores have reached the XCD's L2:
// arrive on XCD x's counter; the XCD's last arriver (of cnt per barrier) runs `leader` and releases the XCD, the others
// spin on the release word, bounded, and raise `wait_code` when the bound runs out.
// err_known: the error word as thread 0 read it a little earlier (~0ull: read it here); once it is up nobody waits.
// POLL_ERR: waiters also look at the error word every 0x400 spins and leave when somebody else has raised it.
template <bool POLL_ERR, typename Leader>
__device__ __forceinline__ void xcd_barrier(GridSync *s, unsigned long long epoch, unsigned x, unsigned long long cnt,
                                            unsigned long long err_known, unsigned long long wait_code, Leader leader) {
  __syncthreads();       // every wave's workgroup-scope release: its stores have reached the XCD's L2
  if (threadIdx.x == 0 && (err_known != ~0ull ? err_known : __hip_atomic_load(&s->error[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const unsigned long long prev = __hip_atomic_fetch_add(&s->xcd_arrive[x][0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev + 1 == cnt * epoch) {
      leader();
      __hip_atomic_store(&s->xcd_release[x][0], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      long spins = 0;
      while (__hip_atomic_load(&s->xcd_release[x][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < epoch) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > GRID_SPIN_LIMIT) { __hip_atomic_store(&s->error[0], wait_code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
        if (POLL_ERR && (spins & 0x3FF) == 0 && __hip_atomic_load(&s->error[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
      }
    }
    asm volatile("s_dcache_inv" ::: "memory");
  }
  __syncthreads();
}

// What an XCD's last arriver does in an all-XCD barrier: write the L2 back, arrive on the global counter, wait for all
// nxcd leaders, invalidate the L2.  false: the wait ran out (error word = code) -- the other XCDs' data is not there.
__device__ __forceinline__ bool xcd_leader_meet(GridSync *s, unsigned long long epoch, unsigned nxcd, unsigned long long code) {
  bool met = true;
  long spins = 0;
  asm volatile("buffer_wbl2 sc1\n\ts_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_fetch_add(&s->global[0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (__hip_atomic_load(&s->global[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned long long)nxcd * epoch) {
    __builtin_amdgcn_s_sleep(1);
    if (++spins > GRID_SPIN_LIMIT) { __hip_atomic_store(&s->error[0], code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); met = false; break; }
  }
  asm volatile("buffer_inv sc1" ::: "memory");
  return met;
}

// epoch = 1, 2, ... over the life of the handle; nxcd = XCDs that hold workgroups
// xcd_cnt: workgroups of this launch on each XCD (the census, passed in the kernel arguments: a load of it here
// would put one more ~1.5 us trip to memory in front of every arrival)
// err_known: the multi-step kernel requests the error word at the start of the phase, off the critical path
__device__ __forceinline__ void grid_barrier(GridSync *s, unsigned long long epoch, unsigned nxcd, const unsigned *xcd_cnt,
                                             unsigned long long err_known = ~0ull) {
  const unsigned x = xcc_id();
  xcd_barrier<false>(s, epoch, x, xcd_cnt[x], err_known, 3ull, [&] { (void)xcd_leader_meet(s, epoch, nxcd, 2ull); });
}

// The barrier of a launch whose workgroups all sit on ONE XCD (steps_kernel's XCD-local mode): they share one L2, so
// there is nothing to write back or invalidate and no second level -- an arrival counter and a release word in that L2.
// (Loads of data another compute unit rewrote still have to pass the reader's L1: the agent-scope loads the multi-step
// kernel uses anyway.)  cnt: workgroups of the launch; x: their XCD.
__device__ __forceinline__ void grid_barrier_local(GridSync *s, unsigned long long epoch, unsigned x, unsigned long long cnt,
                                                   unsigned long long err_known) {
  xcd_barrier<false>(s, epoch, x, cnt, err_known, 3ull, [] {});
}

// ---- the completion ticket ---------------------------------------------------------------------------------------
// Did this workgroup draw the launch's last ticket (workgroup-uniform)?  Called by every workgroup after its last phase;
// the one that gets `true` sees every other workgroup's write-through stores (store_agent) and finishes the launch.
// launch: 0, 1, 2, ... launches that have drawn tickets from `s` before (the counters are monotonic).
// Every block partial of this workgroup went out as a write-through store: once they are acknowledged, take the ticket.
// (Two levels, like the barrier: atomics on ONE address are served at ~15-25 ns apiece, and a flat ticket over
// 500-1000 workgroups that finish together cost 8-12 us here.)
__device__ __forceinline__ bool last_workgroup(GridSync *s, const unsigned *xcd_cnt, unsigned nxcd, unsigned long long launch) {
  __shared__ int done_flag;
  __syncthreads();
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned x = xcc_id();
    const unsigned long long cnt = xcd_cnt[x];
    const unsigned long long t = __hip_atomic_fetch_add(&s->xcd_done[x][0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    done_flag = 0;
    if (t + 1 == (launch + 1) * cnt) {
      const unsigned long long u = __hip_atomic_fetch_add(&s->ticket[2][0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      done_flag = (u + 1 == (launch + 1) * (unsigned long long)nxcd);
    }
    if (done_flag) asm volatile("buffer_inv sc1" ::: "memory");
  }
  __syncthreads();
  return done_flag != 0;
}

// ---- result words ------------------------------------------------------------------------------------------------
// A launch hands its scalars to the host through pinned, host-coherent memory, and the host polls them instead of a
// device-to-host copy + stream synchronisation (20-30 us per round trip on this runtime; the copy alone is a 4 us
// kernel).  The publisher issues NO system-scope fence (an L2 write-back, microseconds), so the words may reach host
// memory in any order: a read counts only when the sequence number AND the checksum match.  One format:
//   [0, k)     the k values of this launch
//   [cap]      checksum = salt ^ seq ^ (k << 56) ^ XOR_q bits(word q) * (2q + 1)
//   [cap + 1]  the launch's sequence number (integer bits; 1, 2, ... per buffer, so the zeroed buffer matches nothing)
// The weights make the checksum see two words that swap or a word that is still last launch's; k under it refuses a
// reader that expects another count.  The three buffers (cap + 2 words each):
constexpr int RES_HOST_K = 6, RES_HOST_CAP = 6;     // res_host (one trial): [0..5) the sums, [5] the barriers' error word
constexpr int STEPS_RES_K = 13, STEPS_RES_CAP = 14; // steps_res (several take_steps): the table is at StepsKernelArgs, trial_kernel.hpp
constexpr int EV_HOST_SLOTS = 32;                   // ev_host (evaluation reductions, k varies by call); >= SCAL_MAX (dist.hpp)
constexpr unsigned long long WORDS_CHECK_SALT = 0xD1B54A32D192ED03ull;

__host__ __device__ __forceinline__ unsigned long long word_bits(double v) { return __builtin_bit_cast(unsigned long long, v); }

// bits(q): the q-th word as 64 bits
template <typename Bits>
__host__ __device__ __forceinline__ unsigned long long words_checksum(int k, unsigned long long seq, Bits bits) {
  unsigned long long ck = WORDS_CHECK_SALT ^ seq ^ ((unsigned long long)k << 56);
  for (int q = 0; q < k; ++q) ck ^= bits(q) * (2ull * (unsigned long long)q + 1ull);
  return ck;
}

// One thread publishes: word(q) yields the q-th value (asked once, in order).  No fence.
// (Host: double or volatile double, as the caller holds the buffer)
template <typename Host, typename Word>
__host__ __device__ __forceinline__ void publish_words(Host *host, int cap, int k, unsigned long long seq, Word word) {
  const unsigned long long ck = words_checksum(k, seq, [&](int q) {      // (one pass: each word is stored as it is summed)
    const double v = word(q);
    host[q] = v;
    return word_bits(v);
  });
  host[cap] = __builtin_bit_cast(double, ck);
  host[cap + 1] = __builtin_bit_cast(double, seq);
}

// Does the buffer hold launch seq's k words, all of them?  Then out[0..k) takes them.  Every word is read through the
// volatile pointer (a plain read in a spin loop may be hoisted) and once (what is checked is what is returned).
inline bool words_ready(const volatile unsigned long long *bits, int cap, int k, unsigned long long seq, double *out) {
  if (k < 0 || k > cap || cap > EV_HOST_SLOTS || bits[cap + 1] != seq) return false;
  unsigned long long w[EV_HOST_SLOTS];
  for (int q = 0; q < k; ++q) w[q] = bits[q];
  if (words_checksum(k, seq, [&](int q) { return w[q]; }) != bits[cap]) return false;
  memcpy(out, w, sizeof(double) * (size_t)k);
  return true;
}

// Wait for launch seq's words: a bounded spin that asks the stream now and then whether the launch has ended, then the
// stream itself and one more look.  998 (message `what`): the launch ended without publishing.
inline int wait_words(hipStream_t stream, const volatile double *host, int cap, int k, unsigned long long seq, double *out,
                      long spin_limit, const char *what) {
  const volatile unsigned long long *bits = reinterpret_cast<const volatile unsigned long long *>(host);
  for (long spin = 0; spin < spin_limit; ++spin) {
    if (words_ready(bits, cap, k, seq, out)) return 0;
    if ((spin & 0xFFFFF) == 0xFFFFF && hipStreamQuery(stream) != hipErrorNotReady) break;
  }
  HIP_TRY(hipStreamSynchronize(stream));
  if (words_ready(bits, cap, k, seq, out)) return 0;
  return fail(998, what);
}

}  // namespace
