// abi_fleet_rescale.hpp -- part of the single translation unit pdhg_hip.hip (included there, inside its extern "C" block, last).
// C ABI: a fleet's RESCALING in one shared launch (include/pdhg_hip_fleet_rescale.h; the kernel in
// fleet_rescale_kernels.hpp; the class in fleet_rescale_eligible, abi_fleet_checks.hpp).  A member of the class rides in
// the launch of fleet_rescale_kernel, one workgroup per member; every other one is served by its own pdhg_rescale and
// pdhg_matrix_max_abs inside the same call, member after member (pdhg_fleet_take_steps_adaptive's convention).
//
// Host side per carried member: what pdhg_rescale does at its entry -- the pending average update settled, the versions
// moved on, room in a retained record for the steps to come -- and one argument block.  No scratch is allocated: the
// factor vectors live in the workgroup's LDS, the results of all members come back through one fleet-owned arena in one
// copy.  The compact bound views are left to their next reader (bnd_dirty, bounds_fresh): one rebuild where pdhg_rescale
// makes one per step.

static FleetRescaleArgs fleet_rescale_block(pdhg_handle *h, double *out) {
  FleetRescaleArgs a{};
  a.n = (int)h->n; a.m = (int)h->m; a.has_q = h->has_q ? 1 : 0; a.retained = h->rs ? 1 : 0;
  a.A = h->A.view(); a.T = h->At.view();
  a.a_val = h->A.val; a.t_val = h->At.val; a.t_nnz = h->At.nnz;
  if (h->has_q) { a.Q = h->Q.view(); a.Qt = h->Qt.view(); a.q_val = h->Q.val; a.qt_val = h->Qt.val; }
  a.c = h->c; a.lb = h->lb; a.ub = h->ub; a.b = h->b;
  if (h->rs) {
    ResolveState &R = *h->rs;
    a.rec = R.rec + R.steps * (h->n + h->m);
    a.rcum_d = R.cum_d; a.rcum_e = R.cum_e;
  }
  a.out = out;
  return a;
}

int pdhg_fleet_rescale(pdhg_handle *fleet, const int *active, int l_inf_ruiz_iterations, int l2_norm_rescaling,
                       int use_pock_chambolle, double pock_chambolle_alpha, double *const *constraint_rescaling_out,
                       double *const *variable_rescaling_out, double *matrix_max_abs_out) {
  RoctxRange roctx_range("pdhg_fleet_rescale");
  if (!fleet) return fail(-1, "null handle");
  if (!fleet_of(fleet)) return fail(-1, "pdhg_fleet_rescale: not a fleet handle");
  // every refusal first: nothing has been touched when one is reported
  if (use_pock_chambolle && !(pock_chambolle_alpha >= 0.0 && pock_chambolle_alpha <= 2.0))
    return fail(-1, "pock_chambolle_alpha must be in [0, 2]");
  if (l_inf_ruiz_iterations < 0) return fail(-1, "pdhg_fleet_rescale: l_inf_ruiz_iterations < 0");
  FleetState &F = *fleet->fleet;
  const int K = (int)F.mem.size();
  int rc;
  std::vector<int> carried, single;
  for (int k = 0; k < K; ++k) {
    if (active && !active[k]) continue;
    pdhg_handle *h = F.mem[(size_t)k];
    if ((rc = check_handle(h))) return rc;
    (fleet_rescale_eligible(h) ? carried : single).push_back(k);
  }
  F.rsc.carried = (int64_t)carried.size();
  F.rsc.single = (int64_t)single.size();
  HIP_TRY(hipSetDevice(fleet->device));
  const FleetRescaleSteps st{l_inf_ruiz_iterations, l2_norm_rescaling ? 1 : 0, use_pock_chambolle ? 1 : 0,
                             use_pock_chambolle ? pock_chambolle_alpha : 0.0};
  const int64_t steps = (int64_t)st.ruiz + st.l2 + st.pock;
  if (!carried.empty()) {
    // the long members start first
    std::stable_sort(carried.begin(), carried.end(), [&](int a, int b) {
      return fleet_member_nnz(F.mem[(size_t)a]) > fleet_member_nnz(F.mem[(size_t)b]);
    });
    size_t words = 0, lds = 0;
    for (int k : carried) {
      pdhg_handle *h = F.mem[(size_t)k];
      if (h->rs && (rc = resolve_reserve(h, steps))) return rc;
      words += (size_t)(h->n + h->m + 1);
      lds = std::max(lds, sizeof(double) * 4 * (size_t)(h->n + h->m));
    }
    if ((rc = fleet_table_reserve(fleet, F.rsc_table, carried.size(), sizeof(FleetRescaleArgs)))) return rc;
    if ((rc = fleet_table_reserve(fleet, F.rsc_out, words, sizeof(double)))) return rc;
    if ((rc = fleet_rescale_lds.raise(fleet->device, lds))) return rc;
    FleetRescaleArgs *table = (FleetRescaleArgs *)F.rsc_table.host;
    size_t placed = 0, off = 0;
    for (int k : carried) {
      pdhg_handle *h = F.mem[(size_t)k];
      const Shards L = shards_of(h);
      if ((rc = flush_pending(L))) return rc;
      bump_version(L);
      h->matrix_version += 1;
      fleet_forget(h);
      table[placed++] = fleet_rescale_block(h, (double *)F.rsc_out.dev + off);
      off += (size_t)(h->n + h->m + 1);
    }
    HIP_TRY(hipMemcpyAsync(F.rsc_table.dev, F.rsc_table.host, sizeof(FleetRescaleArgs) * placed, hipMemcpyHostToDevice, fleet->stream));
    hipLaunchKernelGGL(fleet_rescale_kernel, dim3((unsigned)placed), dim3(FRS_TPB), lds, fleet->stream,
                       (const FleetRescaleArgs *)F.rsc_table.dev, (int)placed, st);
    HIP_TRY(hipGetLastError());
    F.rsc.launches += 1;
    for (int k : carried) {
      pdhg_handle *h = F.mem[(size_t)k];
      if (h->rs) h->rs->steps += steps;
      if (steps > 0) h->bnd_dirty = true;      // lb / ub were rescaled in place: the views are rebuilt where they are next read
    }
    HIP_TRY(hipMemcpyAsync(F.rsc_out.host, F.rsc_out.dev, sizeof(double) * words, hipMemcpyDeviceToHost, fleet->stream));
    HIP_TRY(hipStreamSynchronize(fleet->stream));
    const double *res = (const double *)F.rsc_out.host;
    off = 0;
    for (int k : carried) {
      const pdhg_handle *h = F.mem[(size_t)k];
      const size_t n = (size_t)h->n, m = (size_t)h->m;
      if (variable_rescaling_out && variable_rescaling_out[k] && n > 0) memcpy(variable_rescaling_out[k], res + off, sizeof(double) * n);
      if (constraint_rescaling_out && constraint_rescaling_out[k] && m > 0) memcpy(constraint_rescaling_out[k], res + off + n, sizeof(double) * m);
      if (matrix_max_abs_out) matrix_max_abs_out[k] = res[off + n + m];
      off += n + m + 1;
    }
  }
  for (int k : single) {
    pdhg_handle *h = F.mem[(size_t)k];
    if ((rc = pdhg_rescale(h, l_inf_ruiz_iterations, l2_norm_rescaling, use_pock_chambolle, pock_chambolle_alpha,
                           constraint_rescaling_out ? constraint_rescaling_out[k] : nullptr,
                           variable_rescaling_out ? variable_rescaling_out[k] : nullptr))) return rc;
    if (matrix_max_abs_out && (rc = pdhg_matrix_max_abs(h, matrix_max_abs_out + k))) return rc;
  }
  HIP_TRY(hipStreamSynchronize(fleet->stream));
  return 0;
}

int pdhg_fleet_rescale_info(pdhg_handle *fleet, int64_t out[4]) {
  if (!fleet) return fail(-1, "null handle");
  if (!out) return fail(-1, "out == NULL");
  if (!fleet_of(fleet)) return fail(-1, "pdhg_fleet_rescale_info: not a fleet handle");
  const FleetState &F = *fleet->fleet;
  out[0] = F.rsc.launches; out[1] = F.rsc.carried; out[2] = F.rsc.single; out[3] = F.rsv.other;
  return 0;
}
