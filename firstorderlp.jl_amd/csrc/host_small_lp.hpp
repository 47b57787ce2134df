// host_small_lp.hpp -- part of the single translation unit pdhg_hip.hip (included there, at the place its text used to stand).
// small LPs: a batch of take_steps in one workgroup (small_lp_kernel.hpp): eligibility, staging, launch (host side).

// ---- small LPs: a batch of take_steps in one workgroup, vectors in LDS (small_lp_kernel.hpp) ---------------------
int flush_pending(const Shards &L);
// LDS of a launch: nine n-vectors and four m-vectors; a QP keeps Q x and x' - x as well
size_t small_lp_lds_bytes(const pdhg_handle *h) { return sizeof(double) * ((h->has_q ? 11 : 9) * (size_t)h->n + 4 * (size_t)h->m); }

// A QP (PDHG_SMALL_QP=1; off by default) belongs to the class when both copies of Q suit the kernel as A and A' must:
// row sums of at most SMALL_MAX_ROW entries, plain row blocks.  PDHG_SMALL_LP=0 switches the whole class off.
bool small_lp_eligible(pdhg_handle *h) {
  if (h->small_lp_mode < 0) {
    const char *ev = getenv("PDHG_SMALL_LP"), *qv = getenv("PDHG_SMALL_QP");
    const size_t lds = small_lp_lds_bytes(h);
    bool on = !h->grp && h->n > 0 && h->m > 0 && h->A.segs.empty() && h->At.segs.empty() && !h->A.tiled && !h->At.tiled && h->A.slabs.empty() &&
              h->At.slabs.empty() && h->A.max_row_nnz <= SMALL_MAX_ROW && h->At.max_row_nnz <= SMALL_MAX_ROW &&
              lds <= (size_t)144 * 1024;
    if (h->has_q)
      on = on && qv && qv[0] == '1' && h->Q.segs.empty() && h->Qt.segs.empty() && !h->Q.tiled && !h->Qt.tiled && h->Q.slabs.empty() &&
           h->Qt.slabs.empty() && h->Q.max_row_nnz <= SMALL_MAX_ROW && h->Qt.max_row_nnz <= SMALL_MAX_ROW;
    if (ev) on = on && ev[0] != '0';
    h->small_lp_mode = on ? 1 : 0;
  }
  return h->small_lp_mode == 1 && !h->profile;
}

// The opt-in for the launch's dynamic LDS (beyond 64 KiB), per device and kernel instance; it only ever grows
// (ensure_lds_limit's reasoning).  `policy`: SMALL_ADAPTIVE / _CONSTANT / _MALITSKY_POCK; `which`: 0 the solo
// instantiations, 1 the fleet's; `qp`: the QP form's kernels.
int small_lp_lds_limit(int device, int policy, int which, size_t lds, bool qp = false) {
  static size_t limit[64][3][2][2] = {};
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  size_t &cur = limit[device & 63][policy][which][qp ? 1 : 0];
  if (cur < lds) {
#define SMALL_LDS_OPT_IN(KERNEL)                                                                                               \
  do {                                                                                                                         \
    HIP_TRY(hipFuncSetAttribute((const void *)KERNEL<SMALL_TPB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));        \
    HIP_TRY(hipFuncSetAttribute((const void *)KERNEL<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));              \
  } while (0)
    switch ((policy * 2 + which) * 2 + (qp ? 1 : 0)) {
      case (SMALL_ADAPTIVE * 2 + 0) * 2: SMALL_LDS_OPT_IN(small_lp_steps_kernel); break;
      case (SMALL_ADAPTIVE * 2 + 1) * 2: SMALL_LDS_OPT_IN(small_lp_fleet_kernel); break;
      case (SMALL_CONSTANT * 2 + 0) * 2: SMALL_LDS_OPT_IN(small_lp_constant_kernel); break;
      case (SMALL_CONSTANT * 2 + 1) * 2: SMALL_LDS_OPT_IN(small_fleet_constant_kernel); break;
      case (SMALL_MALITSKY_POCK * 2 + 0) * 2: SMALL_LDS_OPT_IN(small_lp_malitsky_pock_kernel); break;
      case (SMALL_MALITSKY_POCK * 2 + 1) * 2: SMALL_LDS_OPT_IN(small_fleet_malitsky_pock_kernel); break;
      case (SMALL_ADAPTIVE * 2 + 0) * 2 + 1: SMALL_LDS_OPT_IN(small_qp_steps_kernel); break;
      case (SMALL_ADAPTIVE * 2 + 1) * 2 + 1: SMALL_LDS_OPT_IN(small_qp_fleet_kernel); break;
      case (SMALL_CONSTANT * 2 + 0) * 2 + 1: SMALL_LDS_OPT_IN(small_qp_constant_kernel); break;
      default: SMALL_LDS_OPT_IN(small_qp_fleet_constant_kernel); break;      // (no QP reaches here under Malitsky-Pock: policy_handle_check, fleet_stage)
    }
#undef SMALL_LDS_OPT_IN
    cur = lds;
  }
  return 0;
}

// 256 threads up to this many rows / columns, SMALL_TPB beyond (small_lp_kernel.hpp)
bool small_lp_few_rows(const pdhg_handle *h) {
  static const int few_env = dev_env("PDHG_SMALL_FEW_ROWS") ? atoi(dev_env("PDHG_SMALL_FEW_ROWS")) : SMALL_FEW_ROWS;   // dev knob
  return std::max(h->n, h->m) <= few_env;
}

// The argument block of a launch of up to n take_steps of h (solo, or as one entry of a fleet's table): takes the next
// sequence number of the handle's result words and hands the deferred average update to the launch.
SmallLpArgs small_lp_stage(pdhg_handle *h, int n, int max_trials, int table_len, double step_size, double primal_weight,
                           const double *pow_red, const double *pow_growth) {
  SmallLpArgs a{};
  a.n = (int)h->n; a.m = (int)h->m; a.num_eq = (int)h->num_eq;
  a.A = h->A.view(); a.T = h->At.view();
  a.x = h->x; a.y = h->y; a.aty = h->aty; a.sum_x = h->sum_x; a.sum_y = h->sum_y;
  a.c = h->c; a.lb = h->lb; a.ub = h->ub; a.b = h->b;
  a.primal_weight = primal_weight; a.step_size = step_size;
  a.n_steps = n; a.max_trials = max_trials; a.table_len = table_len;
  a.pend = h->pend_x ? 1 : 0; a.pend_w = h->pend_w;
  a.wsum_x = h->sum_x_weights; a.wsum_y = h->sum_y_weights;
  a.pow_red = pow_red; a.pow_growth = pow_growth;
  a.res_host = h->steps_res;
  a.seq = ++h->steps_seq;
  h->pend_x = h->pend_y = false;             // the launch applies it
  return a;
}

// The QP form's block of a staged launch: the same fields and both copies of the objective matrix
SmallQpArgs small_qp_block(const pdhg_handle *h, const SmallLpArgs &a) {
  SmallQpArgs q{};
  static_cast<SmallLpArgs &>(q) = a;
  q.Q = h->Q.view(); q.Qt = h->Qt.view();
  return q;
}

// Wait for launch `seq` of h and take its results into the handle's bookkeeping and the step state (steps_collect).
int small_lp_collect(pdhg_handle *h, unsigned long long seq, StepIO &io) {
  double r[STEPS_RES_K];
  if (int rc = steps_collect(h, seq, io, r)) return rc;
  h->small_lp_launches += 1;
  h->state_version += 1;
  return 0;
}

// What the two solo launchers open with: the class (1: not eligible), the device, the pending term -- the launch consumes
// it; one that only x or only y still owes is applied first -- and the launch's dynamic LDS, opted in for `policy`'s kernel.
static int small_lp_begin(pdhg_handle *h, int policy, size_t *lds) {
  if (!small_lp_eligible(h)) return 1;
  HIP_TRY(hipSetDevice(h->device));
  drop_staging(h);
  if (h->pend_x != h->pend_y) { Shards L = shards_of(h); if (int rc = flush_pending(L)) return rc; }
  *lds = small_lp_lds_bytes(h);
  return small_lp_lds_limit(h->device, policy, 0, *lds, h->has_q);
}

// Up to n_steps take_steps from the step state `io` on, as coop_steps; returns 1 when not eligible (nothing launched)
int small_lp_steps(pdhg_handle *h, int64_t n_steps, StepIO &io) {
  size_t lds = 0;
  int rc = small_lp_begin(h, SMALL_ADAPTIVE, &lds);
  if (rc) return rc;
  const int n = (int)std::min<int64_t>(n_steps, 1 << 20);
  int max_trials = 0, table_len = 0;
  if ((rc = steps_prepare(h, n, io, &max_trials, &table_len))) return rc;
  const SmallLpArgs a = small_lp_stage(h, n, max_trials, table_len, io.step_size, io.primal_weight, h->steps_pow_dev,
                                       h->steps_pow_dev + table_len);
  const auto c1 = std::chrono::steady_clock::now();
  if (h->has_q) {
    const SmallQpArgs q = small_qp_block(h, a);
    if (small_lp_few_rows(h)) hipLaunchKernelGGL(small_qp_steps_kernel<256>, dim3(1), dim3(256), lds, h->stream, q);
    else hipLaunchKernelGGL(small_qp_steps_kernel<SMALL_TPB>, dim3(1), dim3(SMALL_TPB), lds, h->stream, q);
  } else if (small_lp_few_rows(h)) hipLaunchKernelGGL(small_lp_steps_kernel<256>, dim3(1), dim3(256), lds, h->stream, a);
  else hipLaunchKernelGGL(small_lp_steps_kernel<SMALL_TPB>, dim3(1), dim3(SMALL_TPB), lds, h->stream, a);
  HIP_TRY(hipGetLastError());
  const auto c2 = std::chrono::steady_clock::now();
  h->t_launch += std::chrono::duration<double>(c2 - c1).count();
  rc = small_lp_collect(h, a.seq, io);
  h->t_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - c2).count();
  return rc;
}

// ---- the constant and the Malitsky-Pock policy in the same kernel body (PolicyIO, common.hpp) -------------------------
// take_steps of one launch: its worst case -- MALITSKY_POCK_MAX_TRIALS trials in every take_step; one per step under the
// constant policy -- stays within the trials steps_budget allows the largest adaptive launch (steps_collect's time-out
// is sized for that).
int small_policy_launch_steps(int policy, int64_t n_steps) {
  int max_trials = 0, table_len = 0;
  steps_budget(1 << 20, &max_trials, &table_len);
  const int cap = policy == SMALL_MALITSKY_POCK ? max_trials / MALITSKY_POCK_MAX_TRIALS : 1 << 20;
  return (int)std::min<int64_t>(n_steps, std::max(cap, 1));
}

SmallLpArgs small_policy_stage(pdhg_handle *h, int n, const PolicyIO &io) {
  SmallLpArgs a = small_lp_stage(h, n, 0, 0, io.step_size, io.primal_weight, nullptr, nullptr);
  if (io.policy == SMALL_MALITSKY_POCK) {
    a.ratio = io.ratio;
    a.downscaling_factor = io.downscaling_factor; a.breaking_factor = io.breaking_factor;
    a.interpolation_coefficient = io.interpolation_coefficient;
  }
  return a;
}

// Wait for launch `seq` of h; its result words into the handle's bookkeeping and the step state, by the statements of
// the host loops (abi_trial.hpp): half a KKT pass for x' and for every dual trial, a whole one per constant step.
int small_policy_collect(pdhg_handle *h, unsigned long long seq, PolicyIO &io) {
  double r[STEPS_RES_K];
  if (int rc = wait_words(h->stream, h->steps_res, STEPS_RES_CAP, STEPS_RES_K, seq, r, 400000000L,
                          "small-LP kernel finished without publishing its results")) return rc;
  policy_account(h, io, r, r[3]);
  h->small_lp_launches += 1;
  h->state_version += 1;
  return 0;
}

// Up to n_steps take_steps of io.policy in one launch; returns 1 when not eligible (nothing launched).  Malitsky-Pock:
// the caller has seen to it that the primal average is not empty.
int small_policy_steps(pdhg_handle *h, int64_t n_steps, PolicyIO &io) {
  size_t lds = 0;
  int rc = small_lp_begin(h, io.policy, &lds);
  if (rc) return rc;
  if ((rc = steps_result_words(h))) return rc;
  const SmallLpArgs a = small_policy_stage(h, small_policy_launch_steps(io.policy, n_steps), io);
  const bool few = small_lp_few_rows(h);
  const auto c1 = std::chrono::steady_clock::now();
  if (h->has_q) {                           // (the constant policy: Malitsky-Pock has refused the handle, policy_handle_check)
    const SmallQpArgs q = small_qp_block(h, a);
    if (few) hipLaunchKernelGGL(small_qp_constant_kernel<256>, dim3(1), dim3(256), lds, h->stream, q);
    else hipLaunchKernelGGL(small_qp_constant_kernel<SMALL_TPB>, dim3(1), dim3(SMALL_TPB), lds, h->stream, q);
  } else if (io.policy == SMALL_MALITSKY_POCK) {
    if (few) hipLaunchKernelGGL(small_lp_malitsky_pock_kernel<256>, dim3(1), dim3(256), lds, h->stream, a);
    else hipLaunchKernelGGL(small_lp_malitsky_pock_kernel<SMALL_TPB>, dim3(1), dim3(SMALL_TPB), lds, h->stream, a);
  } else {
    if (few) hipLaunchKernelGGL(small_lp_constant_kernel<256>, dim3(1), dim3(256), lds, h->stream, a);
    else hipLaunchKernelGGL(small_lp_constant_kernel<SMALL_TPB>, dim3(1), dim3(SMALL_TPB), lds, h->stream, a);
  }
  HIP_TRY(hipGetLastError());
  const auto c2 = std::chrono::steady_clock::now();
  h->t_launch += std::chrono::duration<double>(c2 - c1).count();
  rc = small_policy_collect(h, a.seq, io);
  h->t_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - c2).count();
  return rc;
}
