// host_trial_coop.hpp -- part of the single translation unit pdhg_hip.hip (included there, at the place its text used to stand).
// the trial step / whole batches of take_steps as ONE persistent kernel (trial_kernel.hpp): grid, census, launch, fallback (host side).

// ---- the trial step as ONE persistent kernel (trial_kernel.hpp) -----------------------------

int coop_prepare(pdhg_handle *h, int cap_limit = 0, bool several_items = false);
bool graph_eligible(pdhg_handle *h);

bool coop_eligible(pdhg_handle *h) {
  if (h->coop_mode < 0) {
    const char *ev = getenv("PDHG_COOP");
    bool on = !h->grp && !h->A.tiled && !h->At.tiled && h->A.slabs.empty() && h->At.slabs.empty() &&
              h->A.segs.empty() && h->At.segs.empty() && h->n > 0 && h->m > 0;
    if (h->has_q) on = on && !h->Q.tiled && !h->Qt.tiled && h->Q.slabs.empty() && h->Qt.slabs.empty();
    if (ev) on = on && ev[0] != '0';
    const char *gv = getenv("PDHG_GRAPH");             // PDHG_GRAPH=0: separate launches, no one-launch path of either kind
    if (gv) on = on && gv[0] != '0';
    h->coop_mode = on ? 1 : 0;
    if (on && coop_prepare(h) != 0) h->coop_mode = 0;  // too many items for one co-resident grid, or no census: graph / plain path
  }
  return h->coop_mode == 1 && !h->profile;
}

// The census of a persistent launch shape: how many of its workgroups the dispatcher places on each XCD (the barriers
// count arrivals per XCD).  census_read: `sync` back from the device once `stream` has drained -- the total, the XCDs
// that hold any, and the count of each; xcd_census: a launch of `grid` registering workgroups first.  What a caller
// makes of a census that does not add up is its own affair.
int census_read(hipStream_t stream, const GridSync *sync, unsigned long long *total, unsigned *nxcd, unsigned cnt[8]) {
  GridSync host;
  HIP_TRY(hipMemcpyAsync(&host, sync, sizeof(GridSync), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  *total = 0;
  *nxcd = 0;
  for (int x = 0; x < 8; ++x) { *total += host.xcd_count[x][0]; *nxcd += host.xcd_count[x][0] > 0; cnt[x] = (unsigned)host.xcd_count[x][0]; }
  return 0;
}
int xcd_census(hipStream_t stream, int grid, GridSync *sync, unsigned long long *total, unsigned *nxcd, unsigned cnt[8]) {
  hipLaunchKernelGGL(xcd_register_kernel, dim3(grid), dim3(TPB), 0, stream, sync);
  HIP_TRY(hipGetLastError());
  return census_read(stream, sync, total, nxcd, cnt);
}
// The handle's all-XCD census (coop_prepare) and what goes with it into the argument block of a persistent launch
// (TrialKernelArgs, StepsKernelArgs).
template <typename Args>
static void census_args(const pdhg_handle *h, Args &a) {
  a.nxcd = h->coop_nxcd; a.relaxed = h->relaxed ? 1 : 0;
  a.trace = h->coop_trace;
  for (int x = 0; x < 8; ++x) a.xcd_cnt[x] = h->coop_xcd_cnt[x];
}
// A barrier of an all-XCD persistent launch (`kernel` names it) ran into its spin limit: the handle's barrier counters are
// out of step now, so it leaves the one-launch paths for good.
static void coop_timed_out(pdhg_handle *h, const char *kernel, double code) {
  h->coop_mode = 0;
  h->coop_fallbacks += 1;
  fprintf(stderr, "[pdhg_hip] %s: a grid barrier timed out (code %g; is the device shared with another "
                  "persistent kernel?) -- this handle uses the %s path from here on\n", kernel, code,
          graph_eligible(h) ? "graph" : "separate-launch");
}

// grid of the persistent launch + the census of workgroups per XCD (once per handle)
// cap_limit: at most this many workgroups (several shards share a device); several_items: accept more items than
// workgroups (the phases then walk several row blocks per workgroup)
int coop_prepare(pdhg_handle *h, int cap_limit, bool several_items) {
  if (h->gsync) return 0;
  HIP_TRY(hipSetDevice(h->device));
  int rc = ensure_result_word(h);
  if (rc) return rc;
  int per_cu = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, trial_kernel<false>, TPB, 0));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, h->device));
  int cap = std::max(8, per_cu * prop.multiProcessorCount / 8 * 8);
  if (const char *ev = dev_env("PDHG_COOP_WGS")) cap = std::max(8, std::min(cap, atoi(ev) / 8 * 8));
  if (cap_limit > 0) cap = std::max(8, std::min(cap, cap_limit / 8 * 8));
  // test knob: pretend the device holds this many workgroups (more than it does: the barriers cannot complete)
  const char *pretend = dev_env("PDHG_COOP_TEST_PRETEND_WGS");
  if (pretend) cap = std::max(8, atoi(pretend) / 8 * 8);
  // one item per workgroup and phase where the device can hold that many: row blocks from the front, long-row chunks from the end
  int items = std::max(h->A.grid + h->A.nchunks, h->At.grid + h->At.nchunks);
  if (h->has_q) items = std::max(items, std::max(h->Q.grid + h->Q.nchunks, h->A.grid + h->A.nchunks + h->Qt.grid + h->Qt.nchunks));
  h->coop_grid = pretend ? cap : std::min(cap, std::max(8, (items + 7) / 8 * 8));
  // More items than co-resident workgroups: the persistent kernel would walk several row blocks per workgroup at
  // 5 workgroups per CU, where the separate stream kernels keep 8 per CU in flight -- measured slower (PageRank-1M,
  // 4 552 items on 1 280 workgroups: 4 380 it/s against 4 620 as a graph of slab passes).  Leave those to the graph.
  if (items > cap && !several_items && !dev_env("PDHG_COOP_FORCE")) {
    h->coop_mode = 0;
    return 1;       // not an error: the caller falls through to the graph / plain path
  }
  HIP_TRY(hipMalloc((void **)&h->gsync, sizeof(GridSync)));
  HIP_TRY(hipMemsetAsync(h->gsync, 0, sizeof(GridSync), h->stream));
  if (getenv("PDHG_COOP_TRACE")) {
    HIP_TRY(hipMalloc((void **)&h->coop_trace, sizeof(unsigned long long) * 8 * (size_t)h->coop_grid));
    HIP_TRY(hipMemsetAsync(h->coop_trace, 0, sizeof(unsigned long long) * 8 * (size_t)h->coop_grid, h->stream));
  }
  unsigned long long total = 0;
  if ((rc = xcd_census(h->stream, h->coop_grid, h->gsync, &total, &h->coop_nxcd, h->coop_xcd_cnt))) return rc;
  if (total != (unsigned long long)h->coop_grid || h->coop_nxcd == 0) {
    h->coop_mode = 0;
    return fail(996, "one-launch trial: workgroup census does not add up");
  }
  if (getenv("PDHG_VERBOSE"))
    fprintf(stderr, "[pdhg_hip] one-launch trial: %d workgroups (%d per CU possible) on %u XCDs, %d + %d / %d + %d row blocks + long chunks\n",
            h->coop_grid, per_cu, h->coop_nxcd, h->A.grid, h->A.nchunks, h->At.grid, h->At.nchunks);
  return 0;
}

TrialProduct trial_product(pdhg_handle *h, CsrDev &D, const double *xin, const EpiArgs &e) {
  TrialProduct P{};
  P.M = D.view();
  P.blks = D.blks; P.nblk = D.nblk; P.per_xcd = D.per_xcd; P.grid = D.grid; P.remap = h->remap ? 1 : 0;
  P.nchunks = D.nchunks; P.nlong = D.nlong; P.long_grid = D.long_grid;
  P.chunk_row = D.chunk_row; P.chunk_off = D.chunk_off; P.chunk_lidx = D.chunk_lidx; P.chunk_partial = D.chunk_partial;
  P.long_ticket = D.long_ticket;
  P.long_row = D.long_row; P.long_chunk_ptr = D.long_chunk_ptr;
  P.xin = xin; P.e = e;
  P.uses = D.coop_uses;
  D.coop_uses += 1;
  return P;
}

// returns 1 when the handle turned out not to suit the one-launch kernel (nothing was launched)
// Two persistent launches that are both only PARTLY resident would wait for each other's workgroups for ever
// (until the spin limit): one such kernel at a time per device, from launch until its results are back.
std::mutex &coop_device_mutex(int device) {
  static std::mutex mu[64];
  return mu[device & 63];
}

int coop_trial(pdhg_handle *h, const TrialArgs &ta, double out[5]) {
  int rc = coop_prepare(h);
  if (rc) return rc;
  const bool xbar_only = !ta.primal;
  std::lock_guard<std::mutex> one_at_a_time(coop_device_mutex(h->device));
  const auto c0 = std::chrono::steady_clock::now();
  TrialKernelArgs a{};
  a.n = (int)h->n; a.xbar_only = xbar_only ? 1 : 0;
  a.x = h->x; a.c = h->c; a.aty = h->aty; a.lb = h->lb; a.ub = h->ub;
  a.tau = ta.step_size / ta.primal_weight; a.theta = ta.theta;
  a.x_next = h->x_next; a.xbar = h->xbar;
  a.avg_w = h->pend_w; a.sum_x = (h->pend_x && !xbar_only) ? h->sum_x : nullptr;
  a.A = trial_product(h, h->A, h->xbar, dual_epilogue(h, ta.primal_weight * ta.step_size));
  a.T = trial_product(h, h->At, h->y_next, aty_epilogue(h));
  a.sp = trial_final_spec(h, h->At.slots(), h->A.slots(), h->has_q ? h->ew_grid_n : 0, h->A.slots(), nullptr);
  a.has_q = h->has_q ? 1 : 0;
  a.epoch = h->coop_epoch;
  h->coop_epoch += 2;
  if (h->has_q) {
    a.q_blocks = h->ew_grid_n;
    a.qx = h->qx; a.dx = h->tmp_n; a.qtdx = h->tmp_n2; a.pq = h->pQ;
    EpiArgs qe{};
    qe.out = h->tmp_n2;
    a.Qtdx = trial_product(h, h->Qt, h->tmp_n, qe);
    if (!xbar_only) {
      qe.out = h->qx;
      a.Qx = trial_product(h, h->Q, h->x, qe);
      h->coop_epoch += 1;
    }
  }
  a.seq_dev = h->seq_dev; a.res_host = h->res_host; a.sync = h->gsync;
  h->seq_expected += 1;
  a.launch = h->coop_launches; a.seq = h->seq_expected;
  census_args(h, a);
  // test knob: raise the barriers' error word in front of launch number k, as a time-out in it would (the launch
  // then runs without synchronisation and reports the error; the recovery below is what is being tested)
  static const long break_at = dev_env("PDHG_COOP_TEST_BREAK_AT") ? atol(dev_env("PDHG_COOP_TEST_BREAK_AT")) : -1;
  if (break_at >= 0 && (long)h->coop_launches == break_at) {
    static const unsigned long long nine = 9ull;
    HIP_TRY(hipMemcpyAsync(&h->gsync->error[0], &nine, sizeof nine, hipMemcpyHostToDevice, h->stream));
  }
  h->coop_launches += 1;
  const auto c1 = std::chrono::steady_clock::now();
  static const bool coh_single = dev_env("PDHG_COOP_COH") && dev_env("PDHG_COOP_COH")[0] == '1';   // dev: L1-bypassing loads in the single-trial kernel too
  if (coh_single) hipLaunchKernelGGL(trial_kernel<true>, dim3(h->coop_grid), dim3(TPB), 0, h->stream, a);
  else hipLaunchKernelGGL(trial_kernel<false>, dim3(h->coop_grid), dim3(TPB), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  const auto c2 = std::chrono::steady_clock::now();
  h->t_set += std::chrono::duration<double>(c1 - c0).count();
  h->t_launch += std::chrono::duration<double>(c2 - c1).count();
  h->n_graph_trials += 1;
  if (!xbar_only) h->pend_x = false;
  h->pend_y = false;                  // the launch carries the deferred average update
  rc = wait_result_word(h, out);
  h->t_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - c2).count();
  if (rc) return rc;
  if (h->res_error != 0.0) {
    // A grid barrier ran into its spin limit: the workgroups were not all co-resident (another process runs a
    // persistent kernel on this device, or a debugger / profiler serialises dispatch).  Once the error word is up no
    // workgroup waits any more, every workgroup still runs every phase, so the launch has ended and the elementwise
    // work that does not depend on the barriers -- the deferred average update it carried -- is applied exactly once.
    // x', y', A'y' and the sums are not trustworthy: the caller repeats the trial on the graph / plain path (its
    // inputs x, y, A'y are untouched), and this handle stays there (coop_timed_out).
    coop_timed_out(h, "one-launch trial", h->res_error);
    return 1;
  }
  return 0;
}

// ---- what the two multi-step launchers (coop_steps, small_lp_steps) share ---------------------------------------
// Trial budget of a launch of n steps, the tables of (total_number_iterations + 1)^-exponent for its trials (host pow,
// uploaded), the pinned result words.  Budget: the steps asked for plus room for rejections (a launch that runs out
// returns at a take_step boundary and the caller launches again); 64 more table entries for finishing the take_step
// the budget ends in.  The tables cost two pow() per entry on the host: sized to the batch, not to the worst case.
// (steps_budget: the budget alone; steps_result_words: the pinned result words alone -- a many-LP launch, host_fleet.hpp,
//  takes both per member and builds ONE pair of tables for all of them)
static void steps_budget(int n, int *max_trials_out, int *table_len_out) {
  int max_trials = n + n / 8 + 16, table_len = max_trials + 64;
  if (const char *tv = dev_env("PDHG_STEPS_TEST_TABLE")) max_trials = table_len = std::max(1, atoi(tv));   // test knob: launches end inside take_steps
  *max_trials_out = max_trials;
  *table_len_out = table_len;
}
static int steps_result_words(pdhg_handle *h) {
  if (!h->steps_res) {
    HIP_TRY(hipHostMalloc((void **)&h->steps_res, STEPS_RES_WORDS * sizeof(double), hipHostMallocCoherent | hipHostMallocMapped));
    memset(h->steps_res, 0, STEPS_RES_WORDS * sizeof(double));
  }
  return 0;
}
static int steps_prepare(pdhg_handle *h, int n, const StepIO &io, int *max_trials_out, int *table_len_out) {
  int max_trials = 0, table_len = 0;
  steps_budget(n, &max_trials, &table_len);
  if (int rc = steps_result_words(h)) return rc;
  if (h->steps_pow_cap < table_len) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->steps_pow_dev) (void)hipFree(h->steps_pow_dev);
    if (h->steps_pow_host) (void)hipHostFree(h->steps_pow_host);
    h->steps_pow_dev = h->steps_pow_host = nullptr;
    h->steps_pow_cap = std::max(table_len, 512);
    HIP_TRY(hipMalloc((void **)&h->steps_pow_dev, sizeof(double) * 2 * (size_t)h->steps_pow_cap));
    HIP_TRY(hipHostMalloc((void **)&h->steps_pow_host, sizeof(double) * 2 * (size_t)h->steps_pow_cap, hipHostMallocDefault));
  }
  // the t-th trial of the launch runs with total_number_iterations = total + t + 1 and uses k1 = that + 1 (pdhg.jl:713-714)
  for (int t = 0; t < table_len; ++t) {
    const double k1 = (double)(io.iterations + t + 2);
    h->steps_pow_host[t] = pow(k1, -io.reduction_exponent);
    h->steps_pow_host[table_len + t] = pow(k1, -io.growth_exponent);
  }
  HIP_TRY(hipMemcpyAsync(h->steps_pow_dev, h->steps_pow_host, sizeof(double) * 2 * (size_t)table_len, hipMemcpyHostToDevice, h->stream));
  *max_trials_out = max_trials;
  *table_len_out = table_len;
  return 0;
}
// Wait for launch `seq` of h and take its result words (the table is at StepsKernelArgs, trial_kernel.hpp) into the
// handle's bookkeeping and the step state: steps and trials, the average's counts and weight sums, step size, iterations,
// KKT passes, steps done, `entry`.  r: the words, for what only one launcher reads.
static int steps_collect(pdhg_handle *h, unsigned long long seq, StepIO &io, double r[STEPS_RES_K]) {
  if (int rc = wait_words(h->stream, h->steps_res, STEPS_RES_CAP, STEPS_RES_K, seq, r, 400000000L,
                          "multi-step kernel finished without publishing its results")) return rc;
  const int64_t steps = (int64_t)r[1], trials = (int64_t)r[2];
  h->n_graph_trials += trials;
  h->sum_x_count += steps; h->sum_y_count += steps;
  h->sum_x_weights = r[6]; h->sum_y_weights = r[7];
  io.step_size = r[0];
  io.iterations += trials;
  io.kkt_passes += (double)trials;
  io.steps_done += steps;
  // (also after a barrier time-out: the launch may have aborted inside a take_step whose earlier trials were rejected,
  //  and the word is written by the same thread as the other result words)
  io.entry = r[12];
  if (r[8] != 0.0) { io.numerical_error = 1; io.steps_done += 1; }   // the failing take_step counts as taken (it is not repeated)
  return 0;
}

// The multi-step kernel's XCD-local mode: LPs whose products are at most PDHG_COOP_LOCAL_MAX (default 32: one per compute
// unit of an XCD) items.  8 x coop_grid workgroups are launched, the dispatcher deals them round the XCDs, those on XCD 0
// work -- the census must find exactly coop_grid of them there.  Own barrier words and epoch (the single-trial kernel
// keeps the handle's all-XCD census).  PDHG_COOP_LOCAL=0 turns it off.  Returns 0 when the mode is on.
static int steps_local_prepare(pdhg_handle *h) {
  if (h->local_mode >= 0) return h->local_mode ? 0 : 1;
  h->local_mode = 0;
  const char *ev = dev_env("PDHG_COOP_LOCAL");
  if (ev && ev[0] == '0') return 1;
  const int cap = dev_env("PDHG_COOP_LOCAL_MAX") ? atoi(dev_env("PDHG_COOP_LOCAL_MAX")) : 32;
  if (h->coop_grid <= 0 || h->coop_grid > cap || dev_env("PDHG_COOP_TEST_PRETEND_WGS")) return 1;
  HIP_TRY(hipMalloc((void **)&h->lsync, sizeof(GridSync)));
  HIP_TRY(hipMemsetAsync(h->lsync, 0, sizeof(GridSync), h->stream));
  unsigned long long total = 0;
  unsigned nxcd = 0, cnt[8];
  if (int rc = xcd_census(h->stream, 8 * h->coop_grid, h->lsync, &total, &nxcd, cnt)) return rc;
  if (cnt[0] != (unsigned)h->coop_grid) return 1;      // the dispatcher dealt them otherwise: all-XCD mode
  h->local_epoch = 0;
  h->local_mode = 1;
  if (getenv("PDHG_VERBOSE"))
    fprintf(stderr, "[pdhg_hip] multi-step kernel: XCD-local mode, %d workgroups on XCD 0 (of %d launched)\n", h->coop_grid, 8 * h->coop_grid);
  return 0;
}

// Does pdhg_take_steps_adaptive take this handle's batches with the multi-step kernel (steps_kernel)?  (The caller has
// checked the handle: a single one, its device current.)
static bool device_loop_for(pdhg_handle *h) {
  // Several take_steps per launch (steps_kernel: the rule on the device; stream-layout LPs on one handle).  Bitwise the
  // per-trial launches (tests/test_gpu_device_loop.py) and faster on every grid measured but one tie: L1-SVM 19.7k ->
  // 23.4k it/s, random 100K 22.5k -> 28.6k, 3000 x 2500 32.7k -> 52.7k (trial_kernel.hpp, profiles/r03_trial_kernel.txt).
  // PDHG_DEVICE_LOOP=0 / 1: never / whenever eligible; PDHG_DEVICE_LOOP_MAX_WGS: largest grid it is the default for.
  // A QP (steps_kernel's QP form) enters with PDHG_DEVICE_LOOP=1 alone: unset, it goes launch by launch as before
  // (profiles/steps_qp_throughput.txt has what the default would have to be decided on).
  const char *dl_env = getenv("PDHG_DEVICE_LOOP");
  bool device_loop = dl_env && dl_env[0] == '1';
  if (!dl_env && !h->profile && !h->has_q && coop_eligible(h)) {
    static const int max_wgs = dev_env("PDHG_DEVICE_LOOP_MAX_WGS") ? atoi(dev_env("PDHG_DEVICE_LOOP_MAX_WGS")) : (1 << 30);
    device_loop = h->coop_grid <= max_wgs;
  }
  return device_loop;
}

// ---- what the two launchers of the persistent multi-step kernels (coop_steps, coop_policy_steps) share -----------------
// Eligibility, staging, the launch and what follows the wait: this text decides whether a handle's barrier counters and
// long-row tickets stay in step after a time-out, so it stands once.  `device_loop`: the launcher's own decision (how
// PDHG_DEVICE_LOOP is read differs between the two).
static bool steps_launch_eligible(pdhg_handle *h, int device_loop) {
  return device_loop && !h->profile && coop_eligible(h) && h->lazy_accept && h->pend_x == h->pend_y;
}

// The StepsKernelArgs part of a launch's argument block (policy_steps_kernel's derives from it) for up to n_steps
// take_steps from (step_size, primal_weight) on; what only one kernel reads -- tables and trial budget, the Malitsky-Pock
// factors -- the launcher adds.  A QP's Q product always goes along; with_qt: Q' too, with dx, Q'dx and the block
// partials of their dot product (the adaptive rule's interaction term).  final_spec: the XCD leaders reduce block
// partials, and read where those are from the control block.  *local_out: the launch takes the XCD-local form.
static int steps_stage(pdhg_handle *h, StepsKernelArgs &a, int n_steps, double step_size, double primal_weight, bool with_qt,
                       bool final_spec, bool *local_out) {
  int rc;
  if (!h->steps_ctl) {
    HIP_TRY(hipMalloc((void **)&h->steps_ctl, sizeof(StepsCtl)));
    HIP_TRY(hipMemsetAsync(h->steps_ctl, 0, sizeof(StepsCtl), h->stream));
  }
  a.n = (int)h->n; a.num_eq = (int)h->num_eq;
  a.xa = h->x; a.xb = h->x_next; a.ya = h->y; a.yb = h->y_next; a.atya = h->aty; a.atyb = h->aty_next;
  a.c = h->c; a.lb = h->lb; a.ub = h->ub; a.b = h->b;
  a.xbar = h->xbar; a.sum_x = h->sum_x; a.sum_y = h->sum_y;
  // trial_product counts one use of the product, as a single trial makes: taken back here, because how many times the
  // launch runs each product -- what its long rows' tickets advance by -- is known only from its results (steps_finish)
  EpiArgs none{};
  a.A = trial_product(h, h->A, nullptr, none);
  a.T = trial_product(h, h->At, nullptr, none);
  h->A.coop_uses -= 1; h->At.coop_uses -= 1;
  a.uses_a = a.A.uses; a.uses_t = a.T.uses;
  a.pA = h->pA; a.pAt = h->pAt; a.pA_slots = h->A.slots(); a.pAt_stride = h->pAt_stride;
  if (h->has_q) {
    // Q x is kept for the iterate and for the trial point (qx / qx2 flip with x).  The kernels compute Q x' beside the
    // other products and never Q x of the iterate they start from: the first trial's Q x is this product, ahead of the
    // launch in stream order -- the bits of trial_kernel's phase -1
    if (!h->qx2 && (rc = alloc_zero(&h->qx2, h->n))) return rc;
    EpiArgs qe{};
    qe.out = h->qx;
    if ((rc = launch_spmv<MODE_PLAIN, 2>(h, h->Q, h->x, qe))) return rc;
    a.Q = trial_product(h, h->Q, nullptr, none);
    h->Q.coop_uses -= 1;
    a.uses_q = a.Q.uses;
    a.qxa = h->qx; a.qxb = h->qx2;
    if (with_qt) {
      a.Qt = trial_product(h, h->Qt, nullptr, none);
      h->Qt.coop_uses -= 1;
      a.uses_qt = a.Qt.uses;
      a.dx = h->tmp_n; a.qtdx = h->tmp_n2; a.pq = h->pQ; a.q_blocks = h->ew_grid_n;
    }
  }
  if (final_spec) {
    const FinalSpec sp = trial_final_spec(h, h->At.slots(), h->A.slots(), a.q_blocks, h->A.slots(), nullptr);
    if (!h->steps_sp_host) HIP_TRY(hipHostMalloc((void **)&h->steps_sp_host, sizeof(FinalSpec), hipHostMallocDefault));
    memcpy(h->steps_sp_host, &sp, sizeof sp);      // (pinned; free again once the launch's results are back)
    HIP_TRY(hipMemcpyAsync(&h->steps_ctl->sp, h->steps_sp_host, sizeof sp, hipMemcpyHostToDevice, h->stream));
  }
  a.primal_weight = primal_weight; a.step_size = step_size;
  a.n_steps = n_steps;
  a.pend = h->pend_x ? 1 : 0; a.pend_w = h->pend_w;
  a.wsum_x = h->sum_x_weights; a.wsum_y = h->sum_y_weights;
  const bool local = steps_local_prepare(h) == 0;
  a.epoch = local ? h->local_epoch : h->coop_epoch;
  a.sync = local ? h->lsync : h->gsync; a.ctl = h->steps_ctl; a.res_host = h->steps_res;
  a.local_g = local ? h->coop_grid : 0; a.local_home = 0;
  // test knob: the kernel expects eight workgroups more than are launched on the home XCD -- its first barrier times out
  if (local && dev_env("PDHG_COOP_LOCAL_TEST_BAD")) a.local_g += 8;
  // The stayers number themselves with a ticket; the word is zeroed before every launch (one 8-byte fill in stream order,
  // once per batch of steps) instead of the host adding coop_grid per launch to a running base: a launch that placed
  // more than the census' workgroups on the home XCD drew more tickets than the host assumed, and every later launch
  // numbered its workers wrongly until the barriers' time-out dropped the mode.
  if (local) {
    HIP_TRY(hipMemsetAsync(&h->lsync->ticket[0][0], 0, sizeof(unsigned long long), h->stream));
    a.local_ticket_base = 0;
  }
  a.seq = ++h->steps_seq;
  census_args(h, a);
  *local_out = local;
  return 0;
}

// The launch itself, in its XCD-local or its all-XCD form; *launched: when the call returned.
template <typename Args>
static int steps_launch(pdhg_handle *h, bool local, void (*local_form)(Args), void (*all_xcd_form)(Args), const Args &a,
                        std::chrono::steady_clock::time_point *launched) {
  const auto c1 = std::chrono::steady_clock::now();
  if (local) hipLaunchKernelGGL(local_form, dim3(8 * h->coop_grid), dim3(TPB), 0, h->stream, a);
  else hipLaunchKernelGGL(all_xcd_form, dim3(h->coop_grid), dim3(TPB), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  *launched = std::chrono::steady_clock::now();
  h->t_launch += std::chrono::duration<double>(*launched - c1).count();
  return 0;
}

// A launch's result words r (the table is at StepsKernelArgs, trial_kernel.hpp) into what the handle keeps about its
// barriers, tickets and vectors; the step state is the launcher's affair.  local, with_qt: as staged; `kernel` names the
// launch in a time-out's message.
static void steps_finish(pdhg_handle *h, const double r[STEPS_RES_K], bool local, bool with_qt, const char *kernel) {
  const int64_t trials = (int64_t)r[2];
  const bool flip = r[3] != 0.0, aborted = r[9] != 0.0 || r[11] != 0.0, qp = h->has_q;
  // products actually run: the counted trials, and after a time-out the trial it rose in and, under Malitsky-Pock,
  // ([9] - 1) more trials of the take_step that the host now takes again from its start (steps_kernel publishes 0 or 1)
  const unsigned long long run = (unsigned long long)trials + (r[9] != 0.0 ? (unsigned long long)r[9] : aborted ? 1ull : 0ull);
  h->steps_launches += 1; h->steps_trials += trials;
  if (local) { h->local_epoch = (unsigned long long)r[10]; h->local_launches += 1; }
  else h->coop_epoch = (unsigned long long)r[10];
  h->A.coop_uses += run;
  h->At.coop_uses += run;
  if (qp) h->Q.coop_uses += run;
  if (qp && with_qt) h->Qt.coop_uses += run;
  if (flip) { std::swap(h->x, h->x_next); std::swap(h->y, h->y_next); std::swap(h->aty, h->aty_next); }
  if (flip && qp) std::swap(h->qx, h->qx2);
  h->pend_x = h->pend_y = r[4] != 0.0;
  h->pend_w = r[5];
  if (run > 0) h->state_version += 1;     // (bump_version of a single handle)
  if (aborted && local) {
    // the XCD-local form failed (a workgroup of the launch was not where the census saw it): the all-XCD form from here on
    h->local_mode = 0;
    fprintf(stderr, "[pdhg_hip] %s, XCD-local mode: a barrier timed out (code %g) -- all-XCD mode from here on\n", kernel, r[11]);
  } else if (aborted) {
    coop_timed_out(h, kernel, r[11]);
  }
}

// Up to n_steps adaptive take_steps in ONE launch (steps_kernel, trial_kernel.hpp), from the step state `io` on.  On
// return io counts the take_steps taken (fewer than n_steps when the launch ran out of its trial budget, met
// numerical_error, or a barrier timed out: the caller goes on from the state left).  Returns 1 when nothing was
// launched (the multi-step kernel is not wanted for this call, or the handle does not suit it).
int coop_steps(pdhg_handle *h, int64_t n_steps, StepIO &io) {
  if (io.device_loop < 0) io.device_loop = device_loop_for(h) ? 1 : 0;
  if (!steps_launch_eligible(h, io.device_loop)) return 1;
  drop_staging(h);      // (the launch consumes the pending term)
  int rc = coop_prepare(h);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const int n = (int)std::min<int64_t>(n_steps, 1 << 20);
  int max_trials = 0, table_len = 0;
  std::lock_guard<std::mutex> one_at_a_time(coop_device_mutex(h->device));
  if ((rc = steps_prepare(h, n, io, &max_trials, &table_len))) return rc;
  const bool qp = h->has_q;
  bool local = false;
  StepsKernelArgs a{};
  if ((rc = steps_stage(h, a, n, io.step_size, io.primal_weight, qp, true, &local))) return rc;
  a.max_trials = max_trials; a.table_len = table_len;
  a.pow_red = h->steps_pow_dev; a.pow_growth = h->steps_pow_dev + table_len;
  std::chrono::steady_clock::time_point c2;
  if (qp) rc = steps_launch(h, local, steps_kernel<true, true>, steps_kernel<false, true>, a, &c2);
  else rc = steps_launch(h, local, steps_kernel<true, false>, steps_kernel<false, false>, a, &c2);
  if (rc) return rc;
  double r[STEPS_RES_K];
  if ((rc = steps_collect(h, a.seq, io, r))) return rc;
  h->t_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - c2).count();
  steps_finish(h, r, local, qp, "multi-step trial kernel");
  return 0;
}

// ---- the constant and the Malitsky-Pock policy in the persistent kernel (policy_steps_kernel, trial_kernel.hpp) -------
// A multi-step launch's result words into the handle's bookkeeping and the step state of the two other policies, by the
// statements of the host loops (abi_trial.hpp): half a KKT pass for x' and for every dual trial, a whole one per constant
// step (halves add exactly: the host loops' bits).  r: the words ([1] take_steps, [2] trials, [6] / [7] weight sums,
// [8] numerical_error, [0] the next take_step's step size); ratio: where the launcher's kernel leaves ratio_step_sizes.
static void policy_account(pdhg_handle *h, PolicyIO &io, const double r[STEPS_RES_K], double ratio) {
  const int64_t steps = (int64_t)r[1], trials = (int64_t)r[2], failed = r[8] != 0.0 ? 1 : 0;
  h->n_graph_trials += trials;
  h->sum_x_count += steps; h->sum_y_count += steps;
  h->sum_x_weights = r[6]; h->sum_y_weights = r[7];
  if (io.policy == SMALL_MALITSKY_POCK) {
    io.step_size = r[0];
    io.ratio = ratio;
    io.iterations += trials;
    for (int64_t q = 0; q < steps + failed + trials; ++q) io.kkt_passes += 0.5;
  } else {
    for (int64_t q = 0; q < steps; ++q) io.kkt_passes += 1;
  }
  io.steps_done += steps + failed;      // the failing take_step counts as taken (it is not repeated), as under the adaptive policy
  if (failed) io.numerical_error = 1;
}

int small_policy_launch_steps(int policy, int64_t n_steps);      // host_small_lp.hpp

// Up to n_steps take_steps of io.policy in ONE launch of policy_steps_kernel, from the step state `io` on; eligibility,
// staging, launch shape and handling of a barrier time-out are the adaptive launcher's (steps_launch_eligible,
// steps_stage, steps_launch, steps_finish).  PDHG_DEVICE_LOOP=1 alone switches it on, for LPs and QPs (read once per
// call); unset or 0, the two policies go launch by launch as before.  Returns 1 when nothing was launched.
// Malitsky-Pock: the caller has seen to it that the primal average is not empty and that the handle is an LP.
int coop_policy_steps(pdhg_handle *h, int64_t n_steps, PolicyIO &io) {
  if (io.device_loop < 0) {
    const char *dl_env = getenv("PDHG_DEVICE_LOOP");
    io.device_loop = dl_env && dl_env[0] == '1' ? 1 : 0;
  }
  if (!steps_launch_eligible(h, io.device_loop)) return 1;
  const bool mp = io.policy == SMALL_MALITSKY_POCK, qp = h->has_q;
  if (mp && qp) return 1;
  drop_staging(h);      // (the launch consumes the pending term)
  int rc = coop_prepare(h);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  if ((rc = steps_result_words(h))) return rc;
  std::lock_guard<std::mutex> one_at_a_time(coop_device_mutex(h->device));
  // (the worst case of a launch -- MALITSKY_POCK_MAX_TRIALS trials in every take_step -- stays within the largest adaptive launch's trials)
  const int n = small_policy_launch_steps(io.policy, n_steps);
  bool local = false;
  PolicyStepsArgs a{};
  // (Malitsky-Pock alone decides on sums: the leaders' second stage reads where the block partials are, as steps_kernel's does)
  if ((rc = steps_stage(h, a, n, io.step_size, io.primal_weight, false, mp, &local))) return rc;
  if (mp) {
    a.ratio = io.ratio;
    a.downscaling_factor = io.downscaling_factor; a.breaking_factor = io.breaking_factor;
    a.interpolation_coefficient = io.interpolation_coefficient;
  }
  std::chrono::steady_clock::time_point c2;
  if (mp) rc = steps_launch(h, local, policy_steps_kernel<true, SMALL_MALITSKY_POCK, false>, policy_steps_kernel<false, SMALL_MALITSKY_POCK, false>, a, &c2);
  else if (qp) rc = steps_launch(h, local, policy_steps_kernel<true, SMALL_CONSTANT, true>, policy_steps_kernel<false, SMALL_CONSTANT, true>, a, &c2);
  else rc = steps_launch(h, local, policy_steps_kernel<true, SMALL_CONSTANT, false>, policy_steps_kernel<false, SMALL_CONSTANT, false>, a, &c2);
  if (rc) return rc;
  h->pend_x = h->pend_y = false;                   // the launch carries the deferred average update
  double r[STEPS_RES_K];
  if ((rc = wait_words(h->stream, h->steps_res, STEPS_RES_CAP, STEPS_RES_K, a.seq, r, 400000000L,
                       "multi-step kernel finished without publishing its results"))) return rc;
  h->t_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - c2).count();
  policy_account(h, io, r, r[12]);
  steps_finish(h, r, local, false, "multi-step policy kernel");
  return 0;
}
