// abi_fleet_checks.hpp -- part of the single translation unit pdhg_hip.hip (included there, after abi_fleet.hpp; what a
// check here shares with one handle's and a batch's stands in host_checks.hpp).
// C ABI: a fleet's CHECKS in shared launches (fleet_check_kernels.hpp): pdhg_eval_point of many members in one call,
// trust-region problems of many members in one call.  A member that suits the one-workgroup kernels rides in the shared
// launch -- a small QP too, with PDHG_SMALL_QP=1, in launches of the QP kernels beside the LPs'; every other one is
// served by its own pdhg_eval_point / pdhg_trust_region_bound inside the same call, member after member
// (pdhg_fleet_take_steps_adaptive's convention).  Either way the result is also left in the member
// (host_fleet.hpp: fleet_store_eval / fleet_store_tr), so the member's own call with the same arguments answers from it.

// Does the member ride in the shared check launches?  An LP on one handle, not profiled, n + m within the one-workgroup
// trust-region kernel's reach, no row of A or A' beyond SMALL_MAX_ROW entries (small_row_sum's order is launch_spmv's up
// to there), plain CSR layouts, and the one-handle evaluation form the kernels restate in force.  Independent of
// small_lp_eligible: the step kernel keeps nine vectors in LDS, these kernels at most three.
// A QP with PDHG_SMALL_QP=1 alone (read per call, like the other switches here), when CSR(Q) suits small_row_sum as A must.
// Q' is not read by a check: a long column of Q keeps a member out of the step class, not out of this one.
static bool fleet_check_eligible(pdhg_handle *h) {
  const char *se = dev_env("PDHG_SMALL_EVAL");
  if (check_handle(h) != 0) return false;
  if (h->has_q) {
    const char *qv = getenv("PDHG_SMALL_QP");
    if (!(qv && qv[0] == '1' && h->Q.max_row_nnz <= SMALL_MAX_ROW && h->Q.segs.empty() && !h->Q.tiled && h->Q.slabs.empty() && h->Q.rowptr))
      return false;
  }
  return !h->grp && !h->profile && h->n + h->m >= 1 && h->n + h->m <= TRS_MAX &&
         h->A.max_row_nnz <= SMALL_MAX_ROW && h->At.max_row_nnz <= SMALL_MAX_ROW && h->A.segs.empty() && h->At.segs.empty() &&
         !h->A.tiled && !h->At.tiled && h->A.slabs.empty() && h->At.slabs.empty() && h->A.rowptr && h->At.rowptr &&
         eval_shared_form_in_force() && !(se && se[0] == '0');
}

// Does the member ride in the shared rescale launch (abi_fleet_rescale.hpp, fleet_rescale_kernel)?  One plain handle, not
// profiled; every resident copy of A, A' (and Q, Q') a plain CSR -- no row segments, no tiled copy, no slabs, no sliced
// jagged copy, no long rows: apply_scaling's scale_one has then one array per matrix to scale, and every row statistic is
// row_op_kernel's alone; n + m within the four factor vectors a workgroup's LDS holds.  LPs and QPs alike, no switch.
static bool fleet_rescale_plain_csr(const CsrDev &D) {
  return D.segs.empty() && !D.tiled && D.slabs.empty() && !D.sj.on() && D.nlong == 0 && (D.rows == 0 || D.rowptr) &&
         (D.nnz == 0 || (D.col && D.val));
}
static bool fleet_rescale_eligible(const pdhg_handle *h) {
  if (h->grp || h->bat || h->owner || h->fleet || h->profile || !h->Achunk.empty()) return false;
  if (h->has_q && !(fleet_rescale_plain_csr(h->Q) && fleet_rescale_plain_csr(h->Qt))) return false;
  return h->n + h->m >= 1 && h->n + h->m <= TRS_MAX && fleet_rescale_plain_csr(h->A) && fleet_rescale_plain_csr(h->At);
}

// a fleet-owned table (device copy, pinned staging) with room for `items` entries of `bytes` each (fleet_reserve's way)
static int fleet_table_reserve(pdhg_handle *f, FleetState::Table &T, size_t items, size_t bytes) {
  if (T.cap >= items * bytes) return 0;
  HIP_TRY(hipStreamSynchronize(f->stream));
  if (T.dev) (void)hipFree(T.dev);
  if (T.host) (void)hipHostFree(T.host);
  T.dev = T.host = nullptr;
  T.cap = 0;
  const size_t cap = std::max<size_t>(2 * items, 64) * bytes;
  HIP_TRY(hipMalloc(&T.dev, cap));
  HIP_TRY(hipHostMalloc(&T.host, cap, hipHostMallocDefault));
  T.cap = cap;
  return 0;
}
// the argument table of check kernel `which`
static int fleet_check_table(pdhg_handle *f, int which, size_t items, size_t bytes) {
  return fleet_table_reserve(f, f->fleet->chk_table[which], items, bytes);
}

// the point items of a call: the LP members' and the QP members', each a launch of its kernel from its table
struct FleetPointItems {
  std::vector<FleetPointArgs> lp;
  std::vector<FleetQpPointArgs> qp;
};

// claim_point of one eligible member, and what the claim asks for -- the average materialised, the products computed -- as
// an item for fleet_point_products_kernel or, for a QP, fleet_qp_point_products_kernel
static int fleet_stage_point(pdhg_handle *h, int point, bool products, FleetPointItems &items, PointClaim *c, CheckMarks &marks) {
  int rc = claim_point(h, point, products, &marks, c);
  if (rc) return rc;
  if (!c->need_div && !c->stale) return 0;
  FleetQpPointArgs a{};
  a.n = (int)h->n; a.m = (int)h->m;
  if (c->need_div) {
    a.do_div = 1;
    a.sum_x = h->sum_x; a.sum_y = h->sum_y; a.wx = h->sum_x_weights; a.wy = h->sum_y_weights;
    a.avg_x = h->px_avg; a.avg_y = h->py_avg;
  }
  a.do_products = c->stale ? 1 : 0;
  a.A = h->A.view(); a.T = h->At.view();
  a.px = c->px; a.py = c->py; a.ax = c->ax; a.aty = c->aty;
  if (h->has_q) {
    a.Q = h->Q.view(); a.qx = c->qx;
    items.qp.push_back(a);
  } else items.lp.push_back(a);      // (the LP part of the block)
  return 0;
}

// upload `items` into table `which` and launch one workgroup per item
extern "C++" template <typename Item, typename Kernel>
static int fleet_check_launch(pdhg_handle *f, int which, const std::vector<Item> &items, Kernel kernel, int threads, size_t lds) {
  if (items.empty()) return 0;
  int rc = fleet_check_table(f, which, items.size(), sizeof(Item));
  if (rc) return rc;
  FleetState &F = *f->fleet;
  memcpy(F.chk_table[which].host, items.data(), sizeof(Item) * items.size());
  HIP_TRY(hipMemcpyAsync(F.chk_table[which].dev, F.chk_table[which].host, sizeof(Item) * items.size(), hipMemcpyHostToDevice, f->stream));
  hipLaunchKernelGGL(kernel, dim3((unsigned)items.size()), dim3(threads), lds, f->stream, (const Item *)F.chk_table[which].dev,
                     (int)items.size());
  HIP_TRY(hipGetLastError());
  F.chk_launches += 1;
  return 0;
}

// the point launches of a call: an empty part issues nothing; every cache marked fresh is filled once both have been issued
static int fleet_point_launches(pdhg_handle *f, const FleetPointItems &items, CheckMarks &marks) {
  int rc;
  if ((rc = fleet_check_launch(f, 0, items.lp, fleet_point_products_kernel, TPB, 0))) return rc;
  if ((rc = fleet_check_launch(f, 3, items.qp, fleet_qp_point_products_kernel, TPB, 0))) return rc;
  marks.issued = true;
  return 0;
}

/* pdhg_eval_point(member k, points[k], out + 24 k) for every k with points[k] >= 0 (pdhg_hip.h). */
int pdhg_fleet_eval_points(pdhg_handle *fleet, const int *points, double *out) {
  RoctxRange roctx_range("pdhg_fleet_eval_points");
  if (!fleet) return fail(-1, "null handle");
  if (!fleet_of(fleet)) return fail(-1, "pdhg_fleet_eval_points: not a fleet handle");
  if (!points || !out) return fail(-1, "null argument");
  FleetState &F = *fleet->fleet;
  const int K = (int)F.mem.size();
  int rc;
  // every argument error first: nothing has been touched when one is reported
  for (int k = 0; k < K; ++k) {
    if (points[k] < 0) continue;
    pdhg_handle *h = F.mem[(size_t)k];
    const std::string who = "pdhg_fleet_eval_points: member " + std::to_string(k);
    if ((rc = check_handle(h))) return rc;
    if (!h->has_original) return fail(-1, who + ": pdhg_set_original_problem has not been called");
    if ((rc = point_error(h, points[k], who))) return rc;
  }
  HIP_TRY(hipSetDevice(fleet->device));
  struct Carried { int k; unsigned long long seq; bool have_avg; };
  std::vector<Carried> carried;
  std::vector<int> single;
  for (int k = 0; k < K; ++k) {
    if (points[k] < 0) continue;
    if (fleet_check_eligible(F.mem[(size_t)k])) carried.push_back(Carried{k, 0ull, false});
    else single.push_back(k);
  }
  F.chk_carried = (int64_t)carried.size();
  F.chk_single = (int64_t)single.size();
  // the long members start first
  std::stable_sort(carried.begin(), carried.end(), [&](const Carried &a, const Carried &b) {
    return F.mem[(size_t)a.k]->n + F.mem[(size_t)a.k]->m > F.mem[(size_t)b.k]->n + F.mem[(size_t)b.k]->m;
  });
  FleetPointItems pitems;
  std::vector<FleetEvalArgs> eitems;
  std::vector<FleetQpEvalArgs> qeitems;
  CheckMarks marks;
  for (Carried &c : carried) {
    pdhg_handle *h = F.mem[(size_t)c.k];
    const int point = points[c.k];
    { Shards L = shards_of(h); if ((rc = flush_pending(L))) return rc; }
    if ((rc = ev_ensure_host(h))) return rc;
    PointClaim pt, av;
    if ((rc = fleet_stage_point(h, point, true, pitems, &pt, marks))) return rc;
    c.have_avg = h->sum_x_count != 0 && h->sum_y_count != 0;
    if (c.have_avg && (rc = fleet_stage_point(h, PDHG_POINT_AVERAGE, false, pitems, &av, marks))) return rc;
    c.seq = ++h->ev_seq;
    const FleetQpEvalArgs a = eval_args_of(h, pt, c.have_avg, h->ev_host, c.seq);
    if (h->has_q) qeitems.push_back(a);
    else eitems.push_back(a);                // (the LP part of the block)
  }
  // at most four launches: the LP members' points, the QP members', the LP evaluations, the QP evaluations
  if ((rc = fleet_point_launches(fleet, pitems, marks))) return rc;
  if ((rc = fleet_check_launch(fleet, 1, eitems, fleet_eval_kernel, TPB, 0))) return rc;
  if ((rc = fleet_check_launch(fleet, 4, qeitems, fleet_qp_eval_kernel, TPB, 0))) return rc;
  for (const Carried &c : carried) {
    pdhg_handle *h = F.mem[(size_t)c.k];
    double r[28];
    if ((rc = ev_wait_host(h, 28, c.seq, r))) return rc;
    double *o = out + (size_t)24 * c.k;
    eval_unpack(h, points[c.k], true, c.have_avg, r, o);
    fleet_store_eval(h, points[c.k], o);
  }
  for (int k : single)
    if ((rc = serve_eval_by_own_call(F.chk_serving, F.mem[(size_t)k], points[k], out + (size_t)24 * k))) return rc;
  return 0;
}

/* pdhg_trust_region_bound(member[i], points[i], ..., out + 8 i) for i < count (pdhg_hip.h). */
int pdhg_fleet_trust_region_bounds(pdhg_handle *fleet, int count, const int *member, const int *points,
                                   const double *primal_weight_norm, const double *dual_weight_norm, const double *radii,
                                   const int *ranges, const int *approximate, double *out) {
  RoctxRange roctx_range("pdhg_fleet_trust_region_bounds");
  if (!fleet) return fail(-1, "null handle");
  if (!fleet_of(fleet)) return fail(-1, "pdhg_fleet_trust_region_bounds: not a fleet handle");
  if (count < 0) return fail(-1, "pdhg_fleet_trust_region_bounds: count < 0");
  if (count == 0) { fleet->fleet->chk_carried = fleet->fleet->chk_single = 0; return 0; }
  if (!member || !points || !primal_weight_norm || !dual_weight_norm || !radii || !ranges || !approximate || !out)
    return fail(-1, "null argument");
  FleetState &F = *fleet->fleet;
  const int K = (int)F.mem.size();
  int rc;
  for (int i = 0; i < count; ++i) {
    const std::string who = "pdhg_fleet_trust_region_bounds: item " + std::to_string(i);
    if (member[i] < 0 || member[i] >= K) return fail(-1, who + ": member index out of range");
    pdhg_handle *h = F.mem[(size_t)member[i]];
    if ((rc = check_handle(h))) return rc;
    if (ranges[i] < 0 || ranges[i] > 2) return fail(-1, who + ": range must be 0, 1 or 2");
    if ((rc = point_error(h, points[i], who))) return rc;
  }
  HIP_TRY(hipSetDevice(fleet->device));
  std::vector<int> carried, single;
  for (int i = 0; i < count; ++i) (fleet_check_eligible(F.mem[(size_t)member[i]]) ? carried : single).push_back(i);
  F.chk_carried = (int64_t)carried.size();
  F.chk_single = (int64_t)single.size();
  std::stable_sort(carried.begin(), carried.end(), [&](int a, int b) {
    const pdhg_handle *ha = F.mem[(size_t)member[a]], *hb = F.mem[(size_t)member[b]];
    return ha->n + ha->m > hb->n + hb->m;
  });
  if (!carried.empty()) {
    const size_t words = (size_t)(EV_HOST_SLOTS + 2);
    // (room to grow into: a fleet's rounds ask for about as many problems each)
    const size_t want = F.chk_res_cap < carried.size() ? std::max<size_t>(2 * carried.size(), 64) : carried.size();
    if ((rc = ensure_result_words(&F.chk_res, &F.chk_res_cap, want, fleet->stream))) return rc;
    FleetPointItems pitems;
    std::vector<TrSmallArgs> titems;
    CheckMarks marks;
    size_t lds = 0;
    const unsigned long long seq = ++F.chk_seq;
    for (size_t j = 0; j < carried.size(); ++j) {
      const int i = carried[j];
      pdhg_handle *h = F.mem[(size_t)member[i]];
      { Shards L = shards_of(h); if ((rc = flush_pending(L))) return rc; }
      PointClaim pt;
      if ((rc = fleet_stage_point(h, points[i], true, pitems, &pt, marks))) return rc;
      TrSmallArgs a{};
      tr_problem_fill(a, h, pt, primal_weight_norm[i], dual_weight_norm[i], radii[i], ranges[i], approximate[i]);
      a.host_out = F.chk_res + j * words;
      a.seq = seq;
      titems.push_back(a);
      lds = std::max(lds, sizeof(double) * 3 * (size_t)(h->n + h->m));
    }
    if ((rc = fleet_tr_lds.raise(fleet->device, lds))) return rc;
    // at most three launches: the LP members' points, the QP members', one trust-region launch for all problems
    if ((rc = fleet_point_launches(fleet, pitems, marks))) return rc;
    if ((rc = fleet_check_launch(fleet, 2, titems, fleet_tr_kernel, TRS_TPB, lds))) return rc;
    for (size_t j = 0; j < carried.size(); ++j) {
      const int i = carried[j];
      if ((rc = wait_words(fleet->stream, F.chk_res + j * words, EV_HOST_SLOTS, 8, seq, out + (size_t)8 * i, 40000000L,
                           "a fleet's trust-region launch finished without publishing its results")))
        return rc;
      fleet_store_tr(F.mem[(size_t)member[i]], points[i], primal_weight_norm[i], dual_weight_norm[i], radii[i], ranges[i],
                     approximate[i], out + (size_t)8 * i);
    }
  }
  for (int i : single)
    if ((rc = serve_tr_by_own_call(F.chk_serving, F.mem[(size_t)member[i]], points[i], primal_weight_norm[i], dual_weight_norm[i],
                                   radii[i], ranges[i], approximate[i], out + (size_t)8 * i)))
      return rc;
  return 0;
}
