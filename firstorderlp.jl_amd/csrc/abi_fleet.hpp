// abi_fleet.hpp -- part of the single translation unit pdhg_hip.hip (included there, inside its extern "C" block).
// C ABI: a fleet of independent small LPs stepped by one launch (host_fleet.hpp, small_lp_fleet_kernel and its two
// siblings for the constant and the Malitsky-Pock policy).
//
// A fleet is a pdhg_handle that runs no iterations of its own: it owns one stream, the argument table and the shared
// tables of powers of the many-LP launch, and its members.  A member is what pdhg_create makes -- its own matrix, its
// own vectors, every single-LP entry point works on it -- on the fleet's device and stream; pdhg_destroy skips it and
// the fleet frees it (the batch's convention, abi_batch.hpp).

static pdhg_handle *fleet_of(pdhg_handle *h) { return (h && h->fleet) ? h : nullptr; }

static void fleet_release(pdhg_handle *h) {
  FleetState *F = h->fleet;
  if (!F) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (pdhg_handle *m : F->mem) destroy_shard(m);
  for (void *p : {(void *)F->args_dev, (void *)F->qargs_dev, (void *)F->pow_dev, F->rsv_dev})
    if (p) (void)hipFree(p);
  for (void *p : {(void *)F->args_host, (void *)F->qargs_host, (void *)F->pow_host, (void *)F->chk_res, F->rsv_host})
    if (p) (void)hipHostFree(p);
  for (FleetState::Table &T : F->chk_table) {
    if (T.dev) (void)hipFree(T.dev);
    if (T.host) (void)hipHostFree(T.host);
  }
  for (FleetState::Table *T : {&F->rsc_table, &F->rsc_out}) {
    if (T->dev) (void)hipFree(T->dev);
    if (T->host) (void)hipHostFree(T->host);
  }
  delete F;
  h->fleet = nullptr;
}

int pdhg_create_fleet(pdhg_handle **out, int device_id, void *stream) {
  if (!out) return fail(-1, "out == NULL");
  *out = nullptr;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (ndev <= 0) return fail(-3, "no HIP device visible");
  int dev = device_id;
  if (dev < 0) HIP_TRY(hipGetDevice(&dev));
  if (dev >= ndev) return fail(-1, "device_id out of range");
  HIP_TRY(hipSetDevice(dev));
  pdhg_handle *h = new pdhg_handle();
  h->self = h;
  h->device = dev;
  if (stream) { h->stream = (hipStream_t)stream; h->own_stream = false; }
  else {
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail((int)e, "hipStreamCreate failed"); }
    h->own_stream = true;
  }
  h->fleet = new FleetState();
  *out = h;
  return 0;
}

int pdhg_fleet_add(pdhg_handle *fleet, int64_t m, int64_t n, int64_t nnz, const int64_t *colptr, const int64_t *rowval,
                   const double *nzval, int index_base, const double *c, const double *b, const double *lb,
                   const double *ub, int64_t num_equalities, pdhg_handle **member) {
  if (!member) return fail(-1, "member == NULL");
  *member = nullptr;
  if (!fleet_of(fleet)) return fail(-1, "pdhg_fleet_add: not a fleet handle");
  pdhg_handle *h = nullptr;
  const int rc = pdhg_create(&h, m, n, nnz, colptr, rowval, nzval, index_base, c, b, lb, ub, num_equalities, fleet->device,
                             (void *)fleet->stream);
  if (rc) return rc;
  if (h->grp) {            // (a row-sharded handle refuses a caller's stream, so pdhg_create never returns one here)
    pdhg_destroy(h);
    return fail(-2, "pdhg_fleet_add: a fleet member must be a single handle");
  }
  h->fleet_of = fleet;
  fleet->fleet->mem.push_back(h);
  *member = h;
  return 0;
}

/* pdhg_take_steps_adaptive(member k, n_steps[k], ...) for every k, the small LPs among them in ONE launch: the members
 * that are small_lp_eligible -- small QPs among them with PDHG_SMALL_QP=1, in launches of the QP kernels beside the LPs'
 * -- and asked for at least 2 steps go into the shared launch (host_fleet.hpp); whatever that
 * launch left of a member -- its trial budget ran out, or its table of powers ended inside a take_step -- and every
 * other member is stepped by pdhg_take_steps_adaptive's own per-handle loop (abi_trial.hpp), in turn. */
int pdhg_fleet_take_steps_adaptive(pdhg_handle *fleet, const int64_t *n_steps, double reduction_exponent,
                                   double growth_exponent, double *step_size, const double *primal_weight,
                                   int64_t *total_number_iterations, double *cumulative_kkt_passes, int *numerical_error,
                                   int64_t *steps_done) {
  RoctxRange roctx_range("pdhg_fleet_take_steps_adaptive");
  if (!fleet) return fail(-1, "null handle");
  if (!fleet_of(fleet)) return fail(-1, "pdhg_fleet_take_steps_adaptive: not a fleet handle");
  if (!n_steps || !step_size || !primal_weight || !total_number_iterations || !cumulative_kkt_passes || !numerical_error ||
      !steps_done)
    return fail(-1, "null argument");
  FleetState &F = *fleet->fleet;
  const int K = (int)F.mem.size();
  for (int k = 0; k < K; ++k)
    if (n_steps[k] < 0) return fail(-2, "pdhg_fleet_take_steps_adaptive: n_steps[" + std::to_string(k) + "] < 0");
  std::vector<StepIO> io;                       // one per member that steps in this call (reserved: the carries point into it)
  io.reserve((size_t)K);
  std::vector<FleetCarry> carry, single;
  for (int k = 0; k < K; ++k) {
    if (n_steps[k] == 0) continue;              // neither read nor written
    numerical_error[k] = 0;
    steps_done[k] = 0;
    io.push_back(StepIO{step_size[k], total_number_iterations[k], cumulative_kkt_passes[k], numerical_error[k], steps_done[k],
                        primal_weight[k], reduction_exponent, growth_exponent});
    pdhg_handle *h = F.mem[(size_t)k];
    FleetCarry c;
    c.k = k;
    c.io = &io.back();
    c.n = (int)std::min<int64_t>(n_steps[k], 1 << 20);
    (n_steps[k] >= 2 && check_handle(h) == 0 && small_lp_eligible(h) ? carry : single).push_back(c);
  }
  F.last_carried = (int64_t)carry.size();
  F.last_single = (int64_t)single.size();
  int rc = fleet_launch(fleet, carry);
  if (rc) return rc;
  // what the shared launch left of a carried member, from where it stopped (the step size on entry of a take_step it
  // ended inside goes to that take_step's accept, as in pdhg_take_steps_adaptive); the others from the start
  for (const std::vector<FleetCarry> *part : {&carry, &single})
    for (const FleetCarry &c : *part) {
      if (c.io->numerical_error || c.io->steps_done >= n_steps[c.k]) continue;
      if ((rc = take_steps_adaptive_resume(F.mem[(size_t)c.k], n_steps[c.k], *c.io))) return rc;
    }
  return 0;
}

/* pdhg_take_steps_constant / pdhg_take_steps_malitsky_pock (member k, n_steps[k], ...) for every k, as
 * pdhg_fleet_take_steps_adaptive does for its policy: the members that are small_lp_eligible and ask for at least 2
 * steps -- under Malitsky-Pock: whose primal average is not empty -- go into the shared launch (fleet_policy_launch);
 * whatever it left of them and every other member is stepped by the per-handle loop (take_steps_policy_resume). */
static int fleet_take_steps_policy(pdhg_handle *fleet, const int64_t *n_steps, std::vector<PolicyIO> &io, const std::vector<int> &member) {
  FleetState &F = *fleet->fleet;
  std::vector<FleetCarry> carry, single;
  for (size_t i = 0; i < io.size(); ++i) {
    const int k = member[i];
    pdhg_handle *h = F.mem[(size_t)k];
    FleetCarry c;
    c.k = k;
    c.pio = &io[i];
    c.n = small_policy_launch_steps(io[i].policy, n_steps[k]);
    const bool quirk = io[i].policy == SMALL_MALITSKY_POCK && h->sum_x_count == 0;
    (n_steps[k] >= 2 && !quirk && check_handle(h) == 0 && small_lp_eligible(h) ? carry : single).push_back(c);
  }
  F.last_carried = (int64_t)carry.size();
  F.last_single = (int64_t)single.size();
  int rc = fleet_policy_launch(fleet, carry);
  if (rc) return rc;
  for (const std::vector<FleetCarry> *part : {&carry, &single})
    for (const FleetCarry &c : *part)
      if ((rc = take_steps_policy_resume(F.mem[(size_t)c.k], n_steps[c.k], *c.pio))) return rc;
  return 0;
}

int pdhg_fleet_take_steps_constant(pdhg_handle *fleet, const int64_t *n_steps, const double *step_size,
                                   const double *primal_weight, double *cumulative_kkt_passes, int64_t *steps_done) {
  RoctxRange roctx_range("pdhg_fleet_take_steps_constant");
  if (!fleet) return fail(-1, "null handle");
  if (!fleet_of(fleet)) return fail(-1, "pdhg_fleet_take_steps_constant: not a fleet handle");
  if (!n_steps || !step_size || !primal_weight || !cumulative_kkt_passes || !steps_done) return fail(-1, "null argument");
  FleetState &F = *fleet->fleet;
  const int K = (int)F.mem.size();
  for (int k = 0; k < K; ++k)
    if (n_steps[k] < 0) return fail(-2, "pdhg_fleet_take_steps_constant: n_steps[" + std::to_string(k) + "] < 0");
  // (what the constant policy neither reads nor writes, per member: PolicyIO binds references)
  std::vector<double> step((size_t)K), ratio((size_t)K, 0.0);
  std::vector<int64_t> iterations((size_t)K, 0);
  std::vector<int> numerical_error((size_t)K, 0);
  std::vector<PolicyIO> io;
  std::vector<int> member;
  io.reserve((size_t)K);
  for (int k = 0; k < K; ++k) {
    if (n_steps[k] == 0) continue;              // neither read nor written
    steps_done[k] = 0;
    step[(size_t)k] = step_size[k];
    io.push_back(PolicyIO{SMALL_CONSTANT, step[(size_t)k], ratio[(size_t)k], iterations[(size_t)k], cumulative_kkt_passes[k],
                          numerical_error[(size_t)k], steps_done[k], primal_weight[k], 0.0, 0.0, 0.0});
    member.push_back(k);
  }
  return fleet_take_steps_policy(fleet, n_steps, io, member);
}

int pdhg_fleet_take_steps_malitsky_pock(pdhg_handle *fleet, const int64_t *n_steps, double downscaling_factor,
                                        double breaking_factor, double interpolation_coefficient, double *step_size,
                                        double *ratio_step_sizes, const double *primal_weight,
                                        int64_t *total_number_iterations, double *cumulative_kkt_passes,
                                        int *numerical_error, int64_t *steps_done) {
  RoctxRange roctx_range("pdhg_fleet_take_steps_malitsky_pock");
  if (!fleet) return fail(-1, "null handle");
  if (!fleet_of(fleet)) return fail(-1, "pdhg_fleet_take_steps_malitsky_pock: not a fleet handle");
  if (!n_steps || !step_size || !ratio_step_sizes || !primal_weight || !total_number_iterations || !cumulative_kkt_passes ||
      !numerical_error || !steps_done)
    return fail(-1, "null argument");
  FleetState &F = *fleet->fleet;
  const int K = (int)F.mem.size();
  for (int k = 0; k < K; ++k) {
    if (n_steps[k] < 0) return fail(-2, "pdhg_fleet_take_steps_malitsky_pock: n_steps[" + std::to_string(k) + "] < 0");
    if (n_steps[k] > 0 && F.mem[(size_t)k]->has_q)
      return fail(-2, "pdhg_fleet_take_steps_malitsky_pock: member " + std::to_string(k) +
                          ": Malitsky and Pock linesearch is only supported for linear programming problems");
  }
  std::vector<PolicyIO> io;
  std::vector<int> member;
  io.reserve((size_t)K);
  for (int k = 0; k < K; ++k) {
    if (n_steps[k] == 0) continue;              // neither read nor written
    numerical_error[k] = 0;
    steps_done[k] = 0;
    io.push_back(PolicyIO{SMALL_MALITSKY_POCK, step_size[k], ratio_step_sizes[k], total_number_iterations[k],
                          cumulative_kkt_passes[k], numerical_error[k], steps_done[k], primal_weight[k], downscaling_factor,
                          breaking_factor, interpolation_coefficient});
    member.push_back(k);
  }
  return fleet_take_steps_policy(fleet, n_steps, io, member);
}

int pdhg_fleet_info(pdhg_handle *fleet, int64_t info[8]) {
  if (!info) return fail(-1, "info == NULL");
  if (!fleet_of(fleet)) return fail(-1, "pdhg_fleet_info: not a fleet handle");
  const FleetState &F = *fleet->fleet;
  for (int q = 0; q < 8; ++q) info[q] = 0;
  info[0] = (int64_t)F.mem.size();
  info[1] = F.launches;
  info[2] = F.last_carried;
  info[3] = F.last_single;
  // the checks in shared launches (abi_fleet_checks.hpp)
  info[4] = F.chk_launches;
  info[5] = F.chk_carried;
  info[6] = F.chk_single;
  info[7] = F.chk_misses;
  return 0;
}
