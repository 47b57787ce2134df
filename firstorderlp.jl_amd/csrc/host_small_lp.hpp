// host_small_lp.hpp -- part of the single translation unit pdhg_hip.hip (included there, at the place its text used to stand).
// small LPs: a batch of take_steps in one workgroup (small_lp_kernel.hpp): eligibility, staging, launch (host side).

// ---- small LPs: a batch of take_steps in one workgroup, vectors in LDS (small_lp_kernel.hpp) ---------------------
int flush_pending(const Shards &L);
bool small_lp_eligible(pdhg_handle *h) {
  if (h->small_lp_mode < 0) {
    const char *ev = getenv("PDHG_SMALL_LP");
    const size_t lds = sizeof(double) * (9 * (size_t)h->n + 4 * (size_t)h->m);
    bool on = !h->grp && !h->has_q && h->n > 0 && h->m > 0 && h->A.segs.empty() && h->At.segs.empty() && !h->A.tiled && !h->At.tiled && h->A.slabs.empty() &&
              h->At.slabs.empty() && h->A.max_row_nnz <= SMALL_MAX_ROW && h->At.max_row_nnz <= SMALL_MAX_ROW &&
              lds <= (size_t)144 * 1024;
    if (ev) on = on && ev[0] != '0';
    h->small_lp_mode = on ? 1 : 0;
  }
  return h->small_lp_mode == 1 && !h->profile;
}

// The opt-in for the launch's dynamic LDS (beyond 64 KiB), per device and kernel instance; it only ever grows
// (ensure_lds_limit's reasoning).  `which`: 0 the solo instantiations, 1 the fleet's.
int small_lp_lds_limit(int device, int which, size_t lds) {
  static size_t limit[64][2] = {};
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  size_t &cur = limit[device & 63][which];
  if (cur < lds) {
    if (which == 0) {
      HIP_TRY(hipFuncSetAttribute((const void *)small_lp_steps_kernel<SMALL_TPB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      HIP_TRY(hipFuncSetAttribute((const void *)small_lp_steps_kernel<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    } else {
      HIP_TRY(hipFuncSetAttribute((const void *)small_lp_fleet_kernel<SMALL_TPB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      HIP_TRY(hipFuncSetAttribute((const void *)small_lp_fleet_kernel<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    cur = lds;
  }
  return 0;
}

size_t small_lp_lds_bytes(const pdhg_handle *h) { return sizeof(double) * (9 * (size_t)h->n + 4 * (size_t)h->m); }

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

// Wait for launch `seq` of h and take its results into the handle's bookkeeping and the step state (steps_collect).
int small_lp_collect(pdhg_handle *h, unsigned long long seq, StepIO &io) {
  double r[STEPS_RES_K];
  if (int rc = steps_collect(h, seq, io, r)) return rc;
  h->small_lp_launches += 1;
  h->state_version += 1;
  return 0;
}

// Up to n_steps take_steps from the step state `io` on, as coop_steps; returns 1 when not eligible (nothing launched)
int small_lp_steps(pdhg_handle *h, int64_t n_steps, StepIO &io) {
  if (!small_lp_eligible(h)) return 1;
  HIP_TRY(hipSetDevice(h->device));
  int rc;
  if (h->pend_x != h->pend_y) { Shards L = shards_of(h); if ((rc = flush_pending(L))) return rc; }
  const int n = (int)std::min<int64_t>(n_steps, 1 << 20);
  int max_trials = 0, table_len = 0;
  if ((rc = steps_prepare(h, n, io, &max_trials, &table_len))) return rc;
  const size_t lds = small_lp_lds_bytes(h);
  if ((rc = small_lp_lds_limit(h->device, 0, lds))) return rc;
  const SmallLpArgs a = small_lp_stage(h, n, max_trials, table_len, io.step_size, io.primal_weight, h->steps_pow_dev,
                                       h->steps_pow_dev + table_len);
  const auto c1 = std::chrono::steady_clock::now();
  if (small_lp_few_rows(h)) hipLaunchKernelGGL(small_lp_steps_kernel<256>, dim3(1), dim3(256), lds, h->stream, a);
  else hipLaunchKernelGGL(small_lp_steps_kernel<SMALL_TPB>, dim3(1), dim3(SMALL_TPB), lds, h->stream, a);
  HIP_TRY(hipGetLastError());
  const auto c2 = std::chrono::steady_clock::now();
  h->t_launch += std::chrono::duration<double>(c2 - c1).count();
  rc = small_lp_collect(h, a.seq, io);
  h->t_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - c2).count();
  return rc;
}
