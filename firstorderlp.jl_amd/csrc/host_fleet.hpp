// host_fleet.hpp -- part of the single translation unit pdhg_hip.hip (included there, after host_small_lp.hpp).
// MANY independent small LPs in one launch (small_lp_fleet_kernel, small_lp_kernel.hpp): the fleet's state and the shared
// launch (host side).  A solo small-LP launch is dim3(1): one of 256 compute units works.  A fleet's launch carries one
// workgroup per member; the members share nothing on the device, so each takes its steps exactly as its solo launch would.
// Small QPs (PDHG_SMALL_QP=1) ride in launches of their own kernels (small_qp_fleet_kernel) beside the LPs', from a table
// of their own blocks (SmallQpArgs).
//
// Per-member host work of a shared launch: one argument block written into a pinned table (uploaded whole, once), no
// pow() of its own -- the members' tables of powers are windows into ONE pair indexed by the absolute
// k1 = total_number_iterations + t + 2 -- and one wait on its own result words.

struct FleetState {
  std::vector<pdhg_handle *> mem;                               // in order of addition; owned
  SmallLpArgs *args_dev = nullptr, *args_host = nullptr;        // the argument table: device copy, pinned staging
  size_t args_cap = 0;
  SmallQpArgs *qargs_dev = nullptr, *qargs_host = nullptr;      // the same for the QP members (the QP form's block)
  size_t qargs_cap = 0;
  double *pow_dev = nullptr, *pow_host = nullptr;               // [2 * pow_cap]: k1^-reduction_exponent, then k1^-growth_exponent
  size_t pow_cap = 0;
  int64_t launches = 0, last_carried = 0, last_single = 0;
  // the checks in shared launches (abi_fleet_checks.hpp): one argument table per kernel (device copy, pinned staging), the
  // fleet-owned result words of the trust-region items (EV_HOST_SLOTS + 2 doubles per item) and their sequence number
  struct Table { void *dev = nullptr, *host = nullptr; size_t cap = 0; } chk_table[5];     // point products, evaluation, trust region; QP point products, QP evaluation
  double *chk_res = nullptr;
  size_t chk_res_cap = 0;
  unsigned long long chk_seq = 0;
  int64_t chk_launches = 0, chk_carried = 0, chk_single = 0, chk_misses = 0;
  bool chk_serving = false;                                     // inside a fleet call's own per-member calls
  // re-solves in shared launches (abi_resolve.hpp): one table per call -- the items, then the members' vectors -- in
  // pinned memory and its device copy; what the calls did (`other`: lazy view rebuilds so far)
  void *rsv_dev = nullptr, *rsv_host = nullptr;
  size_t rsv_cap = 0;
  ResolveCounters rsv;
  // the rescaling in one shared launch (abi_fleet_rescale.hpp): the argument table, the arena the members' factors and
  // max |a| come back in (device, pinned copy) and what the calls did (`other` unused: the view rebuilds are rsv's)
  Table rsc_table, rsc_out;
  ResolveCounters rsc;
};

// ---- what a fleet's check calls leave in a member (pdhg_handle::fc_eval / fc_tr): pdhg_eval_point and
// pdhg_trust_region_bound on the member answer from them, without a launch, while the member's state, restart point and
// matrix are those of the fleet call and the arguments are the same bits.
inline bool fleet_versions_hold(const pdhg_handle *h, const uint64_t v[3]) {
  return v[0] == h->state_version && v[1] == h->restart_version && v[2] == h->matrix_version;
}
inline uint64_t fleet_bits(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }

bool fleet_stored_eval(pdhg_handle *h, int point, double out[24]) {
  const pdhg_handle::FleetEvalResult &r = h->fc_eval;
  if (!r.valid || r.point != point || !fleet_versions_hold(h, r.version)) return false;
  for (int q = 0; q < 24; ++q) out[q] = r.out[q];
  // (what pdhg_eval_point leaves for pdhg_distance_to_restart / pdhg_point_sumsq)
  for (int q = 0; q < 6; ++q) h->chk_vals[q] = r.chk_vals[q];
  h->chk_state = h->state_version; h->chk_restart = h->restart_version; h->chk_point = point; h->chk_have_avg = r.have_avg;
  return true;
}
void fleet_store_eval(pdhg_handle *h, int point, const double out[24]) {
  pdhg_handle::FleetEvalResult &r = h->fc_eval;
  r.valid = h->chk_state == h->state_version && h->chk_restart == h->restart_version && h->chk_point == point;   // (the prefetch ran)
  r.point = point;
  r.version[0] = h->state_version; r.version[1] = h->restart_version; r.version[2] = h->matrix_version;
  for (int q = 0; q < 24; ++q) r.out[q] = out[q];
  for (int q = 0; q < 6; ++q) r.chk_vals[q] = h->chk_vals[q];
  r.have_avg = h->chk_have_avg;
}
static bool fleet_tr_same(const pdhg_handle *h, const pdhg_handle::FleetTrResult &r, int point, double wp, double wd,
                          double radius, int range, int approximate) {
  return r.valid && r.point == point && r.range == range && r.approximate == (approximate ? 1 : 0) && r.wp == fleet_bits(wp) &&
         r.wd == fleet_bits(wd) && r.radius == fleet_bits(radius) && fleet_versions_hold(h, r.version);
}
bool fleet_stored_tr(pdhg_handle *h, int point, double wp, double wd, double radius, int range, int approximate, double out[8]) {
  for (const pdhg_handle::FleetTrResult &r : h->fc_tr)
    if (fleet_tr_same(h, r, point, wp, wd, radius, range, approximate)) {
      for (int q = 0; q < 8; ++q) out[q] = r.out[q];
      return true;
    }
  return false;
}
void fleet_store_tr(pdhg_handle *h, int point, double wp, double wd, double radius, int range, int approximate, const double out[8]) {
  pdhg_handle::FleetTrResult *slot = nullptr;
  for (pdhg_handle::FleetTrResult &r : h->fc_tr)                      // the same problem again, or a result that went stale
    if (!slot && (fleet_tr_same(h, r, point, wp, wd, radius, range, approximate) || !r.valid || !fleet_versions_hold(h, r.version))) slot = &r;
  if (!slot) { slot = &h->fc_tr[h->fc_tr_next]; h->fc_tr_next = (h->fc_tr_next + 1) % pdhg_handle::FC_TR_SLOTS; }
  slot->valid = true; slot->point = point; slot->range = range; slot->approximate = approximate ? 1 : 0;
  slot->wp = fleet_bits(wp); slot->wd = fleet_bits(wd); slot->radius = fleet_bits(radius);
  slot->version[0] = h->state_version; slot->version[1] = h->restart_version; slot->version[2] = h->matrix_version;
  for (int q = 0; q < 8; ++q) slot->out[q] = out[q];
}
// what the three versions do not see: the evaluation also reads the original problem (E, Dv, b_o, c_o, lb_o, ub_o), so
// pdhg_set_original_problem forgets the stored results
void fleet_forget(pdhg_handle *h) {
  h->fc_eval.valid = false;
  for (pdhg_handle::FleetTrResult &r : h->fc_tr) r.valid = false;
}
// a pdhg_eval_point / pdhg_trust_region_bound call on a member that no stored result answered -- the caller's calls only:
// the calls by which a fleet call itself serves a member it does not carry (chk_serving) are no misses
void fleet_count_miss(pdhg_handle *h) {
  if (h->fleet_of && h->fleet_of->fleet && !h->fleet_of->fleet->chk_serving) h->fleet_of->fleet->chk_misses += 1;
}
// The same path for a batch's member (`owner` = the batch; pdhg_batch_eval_points stores its results as a fleet's call
// does): is the handle a member whose group can have left a result in it, and the group's counts of evaluations answered
// from one / launched by the member although the batch had been asked
inline bool stored_checks_member(const pdhg_handle *h) { return h->fleet_of != nullptr || h->owner != nullptr; }
void stored_eval_served(pdhg_handle *h) {
  if (h->owner) h->owner->bchk_served += 1;
}
void stored_eval_missed(pdhg_handle *h) {
  fleet_count_miss(h);
  if (h->owner && h->owner->bchk_asked && !h->owner->bchk_serving) h->owner->bchk_misses += 1;
}

// one carried member of a call
struct FleetCarry {
  int k = 0;                   // index in FleetState::mem
  StepIO *io = nullptr;        // its step state (bound to the caller's arrays at k)
  PolicyIO *pio = nullptr;     // ... under the constant or the Malitsky-Pock policy (fleet_policy_launch)
  int n = 0, max_trials = 0, table_len = 0;
  int64_t k1_first = 0;        // k1 of its first trial
  bool few = false;
  unsigned long long seq = 0;
};

int fleet_reserve(pdhg_handle *f, size_t members, size_t qp_members, size_t span) {
  FleetState &F = *f->fleet;
  if (F.args_cap < members) {
    HIP_TRY(hipStreamSynchronize(f->stream));
    if (F.args_dev) (void)hipFree(F.args_dev);
    if (F.args_host) (void)hipHostFree(F.args_host);
    F.args_dev = F.args_host = nullptr;
    F.args_cap = 0;
    const size_t cap = std::max<size_t>(2 * members, 64);
    HIP_TRY(hipMalloc((void **)&F.args_dev, sizeof(SmallLpArgs) * cap));
    HIP_TRY(hipHostMalloc((void **)&F.args_host, sizeof(SmallLpArgs) * cap, hipHostMallocDefault));
    F.args_cap = cap;
  }
  if (F.qargs_cap < qp_members) {
    HIP_TRY(hipStreamSynchronize(f->stream));
    if (F.qargs_dev) (void)hipFree(F.qargs_dev);
    if (F.qargs_host) (void)hipHostFree(F.qargs_host);
    F.qargs_dev = F.qargs_host = nullptr;
    F.qargs_cap = 0;
    const size_t cap = std::max<size_t>(2 * qp_members, 64);
    HIP_TRY(hipMalloc((void **)&F.qargs_dev, sizeof(SmallQpArgs) * cap));
    HIP_TRY(hipHostMalloc((void **)&F.qargs_host, sizeof(SmallQpArgs) * cap, hipHostMallocDefault));
    F.qargs_cap = cap;
  }
  if (F.pow_cap < span) {
    HIP_TRY(hipStreamSynchronize(f->stream));
    if (F.pow_dev) (void)hipFree(F.pow_dev);
    if (F.pow_host) (void)hipHostFree(F.pow_host);
    F.pow_dev = F.pow_host = nullptr;
    F.pow_cap = 0;
    const size_t cap = std::max<size_t>(2 * span, 1024);
    HIP_TRY(hipMalloc((void **)&F.pow_dev, sizeof(double) * 2 * cap));
    HIP_TRY(hipHostMalloc((void **)&F.pow_host, sizeof(double) * 2 * cap, hipHostMallocDefault));
    F.pow_cap = cap;
  }
  return 0;
}

// The parts of a shared launch, in the order of the tables: the LP members in one table, the QP members in the other; in
// each the members of up to SMALL_FEW_ROWS rows and columns (256 threads) before the others (SMALL_TPB), the solo rule;
// each part by descending nnz, Q's entries counted (the long members start first, the tail is short).
struct FleetParts {
  size_t count[2][2] = {};     // [QP][SMALL_TPB threads]
  size_t lds[2][2] = {};       // the largest member's dynamic LDS
};
static int64_t fleet_member_nnz(const pdhg_handle *h) { return h->nnz + (h->has_q ? h->Q.nnz : 0); }
static size_t fleet_qp_members(const FleetState &F, const std::vector<FleetCarry> &carry) {
  size_t k = 0;
  for (const FleetCarry &c : carry) k += F.mem[(size_t)c.k]->has_q ? 1 : 0;
  return k;
}

// Orders `carry` (every c.few set), writes every member's block -- stage(c, h): its SmallLpArgs, which takes the
// member's next sequence number -- into the table of its kind, opts the kernels of `policy` in for the parts' LDS and
// queues the upload of the tables.
template <class Stage>
int fleet_stage(pdhg_handle *f, std::vector<FleetCarry> &carry, int policy, FleetParts &P, Stage stage) {
  FleetState &F = *f->fleet;
  // Malitsky-Pock takes LPs only (pdhg.jl; the callers have refused the call already): before anything is staged
  if (policy == SMALL_MALITSKY_POCK && fleet_qp_members(F, carry) > 0)
    return fail(-2, "the one-workgroup kernel has no Malitsky-Pock form for QPs");
  std::stable_sort(carry.begin(), carry.end(), [&](const FleetCarry &a, const FleetCarry &b) {
    const pdhg_handle *ha = F.mem[(size_t)a.k], *hb = F.mem[(size_t)b.k];
    if (ha->has_q != hb->has_q) return hb->has_q;
    if (a.few != b.few) return a.few;
    return fleet_member_nnz(ha) > fleet_member_nnz(hb);
  });
  size_t placed[2] = {0, 0};
  for (FleetCarry &c : carry) {
    pdhg_handle *h = F.mem[(size_t)c.k];
    const int qp = h->has_q ? 1 : 0, big = c.few ? 0 : 1;
    const SmallLpArgs a = stage(c, h);
    c.seq = a.seq;
    if (qp) F.qargs_host[placed[1]++] = small_qp_block(h, a);
    else F.args_host[placed[0]++] = a;
    P.count[qp][big] += 1;
    P.lds[qp][big] = std::max(P.lds[qp][big], small_lp_lds_bytes(h));
  }
  int rc;
  for (int qp = 0; qp < 2; ++qp)
    if (placed[qp] > 0 && (rc = small_lp_lds_limit(f->device, policy, 1, std::max(P.lds[qp][0], P.lds[qp][1]), qp != 0))) return rc;
  if (placed[0] > 0) HIP_TRY(hipMemcpyAsync(F.args_dev, F.args_host, sizeof(SmallLpArgs) * placed[0], hipMemcpyHostToDevice, f->stream));
  if (placed[1] > 0) HIP_TRY(hipMemcpyAsync(F.qargs_dev, F.qargs_host, sizeof(SmallQpArgs) * placed[1], hipMemcpyHostToDevice, f->stream));
  return 0;
}

// The launches of the staged parts, back to back: at most four (LP / QP x 256 / SMALL_TPB threads), each over its stretch
// of its table.
int fleet_launch_parts(pdhg_handle *f, int policy, const FleetParts &P) {
  FleetState &F = *f->fleet;
#define FLEET_GO(KERNEL, TABLE)                                                                                    \
  do {                                                                                                             \
    if (big) hipLaunchKernelGGL(KERNEL<SMALL_TPB>, dim3((unsigned)cnt), dim3(SMALL_TPB), lds, f->stream, TABLE, (int)cnt);   \
    else hipLaunchKernelGGL(KERNEL<256>, dim3((unsigned)cnt), dim3(256), lds, f->stream, TABLE, (int)cnt);                   \
  } while (0)
  for (int qp = 0; qp < 2; ++qp) {
    size_t first = 0;
    for (int big = 0; big < 2; ++big) {
      const size_t cnt = P.count[qp][big], lds = P.lds[qp][big];
      if (cnt == 0) continue;
      const SmallLpArgs *lp_table = F.args_dev + (qp ? 0 : first);
      const SmallQpArgs *qp_table = F.qargs_dev + (qp ? first : 0);
      if (qp) {
        if (policy == SMALL_CONSTANT) FLEET_GO(small_qp_fleet_constant_kernel, qp_table);      // (fleet_stage admits no QP under Malitsky-Pock)
        else FLEET_GO(small_qp_fleet_kernel, qp_table);
      } else {
        if (policy == SMALL_MALITSKY_POCK) FLEET_GO(small_fleet_malitsky_pock_kernel, lp_table);
        else if (policy == SMALL_CONSTANT) FLEET_GO(small_fleet_constant_kernel, lp_table);
        else FLEET_GO(small_lp_fleet_kernel, lp_table);
      }
      F.launches += 1;
      first += cnt;
    }
  }
#undef FLEET_GO
  HIP_TRY(hipGetLastError());
  return 0;
}

// The shared launch of `carry` (every entry small_lp_eligible, n >= 2): at most four kernel launches back to back
// (FleetParts), then one wait per member.  On return every member's step state holds what small_lp_steps would have left
// in it.
int fleet_launch(pdhg_handle *f, std::vector<FleetCarry> &carry) {
  FleetState &F = *f->fleet;
  if (carry.empty()) return 0;
  const double reduction_exponent = carry[0].io->reduction_exponent, growth_exponent = carry[0].io->growth_exponent;   // the call's
  HIP_TRY(hipSetDevice(f->device));
  int rc;
  // the tables of powers: one pair for the call, from the smallest to the largest k1 a member can reach
  int64_t lo = INT64_MAX, hi = 0;
  for (FleetCarry &c : carry) {
    pdhg_handle *h = F.mem[(size_t)c.k];
    drop_staging(h);      // (the launch consumes the pending term)
    if (h->pend_x != h->pend_y) { Shards L = shards_of(h); if ((rc = flush_pending(L))) return rc; }
    if ((rc = steps_result_words(h))) return rc;
    steps_budget(c.n, &c.max_trials, &c.table_len);
    c.k1_first = c.io->iterations + 2;      // (steps_prepare: trial t of the launch uses k1 = total + t + 2)
    c.few = small_lp_few_rows(h);
    lo = std::min(lo, c.k1_first);
    hi = std::max(hi, c.k1_first + c.table_len);          // one past the last
  }
  const size_t span = (size_t)(hi - lo);
  if ((rc = fleet_reserve(f, carry.size(), fleet_qp_members(F, carry), span))) return rc;
  {
    // every entry a member can read is the host pow() steps_prepare computes; entries no member covers stay as they are
    std::vector<std::pair<int64_t, int64_t>> iv;
    for (const FleetCarry &c : carry) iv.emplace_back(c.k1_first, c.k1_first + c.table_len);
    std::sort(iv.begin(), iv.end());
    int64_t done_to = lo;
    for (const auto &v : iv) {
      for (int64_t k1 = std::max(done_to, v.first); k1 < v.second; ++k1) {
        F.pow_host[(size_t)(k1 - lo)] = pow((double)k1, -reduction_exponent);
        F.pow_host[span + (size_t)(k1 - lo)] = pow((double)k1, -growth_exponent);
      }
      done_to = std::max(done_to, v.second);
    }
    HIP_TRY(hipMemcpyAsync(F.pow_dev, F.pow_host, sizeof(double) * 2 * span, hipMemcpyHostToDevice, f->stream));
  }
  FleetParts P;
  if ((rc = fleet_stage(f, carry, SMALL_ADAPTIVE, P, [&](const FleetCarry &c, pdhg_handle *h) {
         const size_t off = (size_t)(c.k1_first - lo);
         return small_lp_stage(h, c.n, c.max_trials, c.table_len, c.io->step_size, c.io->primal_weight, F.pow_dev + off,
                               F.pow_dev + span + off);
       }))) return rc;
  if ((rc = fleet_launch_parts(f, SMALL_ADAPTIVE, P))) return rc;
  for (const FleetCarry &c : carry)
    if ((rc = small_lp_collect(F.mem[(size_t)c.k], c.seq, *c.io))) return rc;
  return 0;
}

// The same for the constant and the Malitsky-Pock policy (every entry small_lp_eligible, n >= 2, Malitsky-Pock: a primal
// average that is not empty): no tables of powers, the policy's own kernels, what small_policy_steps would have left.
int fleet_policy_launch(pdhg_handle *f, std::vector<FleetCarry> &carry) {
  FleetState &F = *f->fleet;
  if (carry.empty()) return 0;
  const int policy = carry[0].pio->policy;
  HIP_TRY(hipSetDevice(f->device));
  int rc;
  for (FleetCarry &c : carry) {
    pdhg_handle *h = F.mem[(size_t)c.k];
    drop_staging(h);      // (the launch consumes the pending term)
    if (h->pend_x != h->pend_y) { Shards L = shards_of(h); if ((rc = flush_pending(L))) return rc; }
    if ((rc = steps_result_words(h))) return rc;
    c.few = small_lp_few_rows(h);
  }
  if ((rc = fleet_reserve(f, carry.size(), fleet_qp_members(F, carry), 0))) return rc;
  FleetParts P;
  if ((rc = fleet_stage(f, carry, policy, P, [&](const FleetCarry &c, pdhg_handle *h) { return small_policy_stage(h, c.n, *c.pio); })))
    return rc;
  if ((rc = fleet_launch_parts(f, policy, P))) return rc;
  for (const FleetCarry &c : carry)
    if ((rc = small_policy_collect(F.mem[(size_t)c.k], c.seq, *c.pio))) return rc;
  return 0;
}
