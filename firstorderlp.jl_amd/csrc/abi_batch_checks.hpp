// abi_batch_checks.hpp -- part of the single translation unit pdhg_hip.hip (included there, inside its extern "C" block, after
// abi_batch_resolve.hpp; what a check here shares with one handle's and a fleet's stands in host_checks.hpp).
// C ABI: a batch's CHECKS in shared launches (include/pdhg_hip_batch_checks.h; kernels in batch_check_kernels.hpp).
//
//   pdhg_batch_point_products   A x, A' y (and Q x) at points of many members: one pass per point kind -- the points packed
//                               member-interleaved into the batch's X / Y, then one plain batched product per matrix
//                               straight into the members' per-point caches, whose keys claim_point sets as it does for
//                               the member's own point_products: that call then finds them fresh and launches nothing
//   pdhg_batch_eval_points      the products, then pdhg_eval_point's one-handle form of all carried members in four
//                               launches; every result is stored with its member (host_fleet.hpp: fleet_store_eval)
//   pdhg_batch_check_info       what the calls did
//
// X / Y are scratch between trials: every trial writes the lanes of its active members (batch_primal_kernel or
// batch_pack_kernel, then the dual epilogue) before a product gathers them, masked lanes are never read, and the warm start
// borrows Y the same way.  A product of the batch with long rows (BatchProduct::nlong > 0) is taken by each member's own
// launch_spmv: the batched long-row chunks are another summation order, and these calls promise the member's bits.

static int batch_checks_ensure(pdhg_handle *h) {
  BatchState::Checks &C = h->bat->chk;
  if (C.stage_dev) return 0;
  size_t cap = C.res ? BATCH_MAX : 0;
  int rc = ensure_result_words(&C.res, &cap, BATCH_MAX, h->stream);
  if (rc) return rc;
  HIP_TRY(hipHostMalloc((void **)&C.stage_host, sizeof(BatchCheckStage), hipHostMallocDefault));
  HIP_TRY(hipEventCreateWithFlags(&C.uploaded, hipEventDisableTiming));
  HIP_TRY(hipMalloc((void **)&C.stage_dev, sizeof(BatchCheckStage)));
  return 0;
}

// the entries and masks of one call, pass by pass (pass p = point kind p: CURRENT, AVERAGE, RESTART)
struct BatchCheckCall {
  int count[3] = {0, 0, 0};             // entries of BatchCheckStage::pts[p]
  unsigned mask[3] = {0, 0, 0};         // members whose products pass p computes
  int slot[3][BATCH_MAX];               // member k's entry of pass p, or -1
  PointRef pt[3][BATCH_MAX];            // where mask[p] names member k: the point and where its products go
  BatchCheckCall() { for (auto &row : slot) for (int &s : row) s = -1; }
};

// every argument error of one (member, point), before anything is touched
static int batch_check_refuse(pdhg_handle *h, int k, int point, const std::string &who) {
  BatchState &B = *h->bat;
  if (k < 0 || k >= B.K) return fail(-1, who + ": member index out of range");
  pdhg_handle *m = B.mem[(size_t)k];
  int rc = check_handle(m);
  if (rc) return rc;
  return point_error(m, point, who);
}

// claim_point of member k at `point`, and what the claim asks for -- the average materialised, the products computed -- as
// an entry of the point's pass.  products == false: the average only (the evaluation's distances).
static int batch_check_stage(pdhg_handle *h, int k, int point, bool products, BatchCheckStage &S, BatchCheckCall &call,
                             CheckMarks &marks, PointClaim *c) {
  pdhg_handle *m = h->bat->mem[(size_t)k];
  const int p = point_index(point);
  int rc = claim_point(m, point, products, &marks, c);
  if (rc) return rc;
  if (!c->need_div && !c->stale) return 0;
  int &slot = call.slot[p][k];
  if (slot < 0) {
    slot = call.count[p]++;
    BatchCheckPoint e{};
    e.k = k;
    e.src_x = c->px; e.src_y = c->py;
    if (c->need_div) {
      e.do_div = 1;
      e.src_x = m->sum_x; e.src_y = m->sum_y; e.wx = m->sum_x_weights; e.wy = m->sum_y_weights;
      e.avg_x = m->px_avg; e.avg_y = m->py_avg;
    }
    S.pts[p][slot] = e;
  }
  if (c->stale) {
    S.pts[p][slot].pack = 1;
    call.mask[p] |= 1u << k;
    call.pt[p][k] = *c;
    S.out[p][0][k] = c->ax; S.out[p][1][k] = c->aty; S.out[p][2][k] = c->qx;
  }
  return 0;
}

// before the staging buffer is written again: the last call's upload has been read
static int batch_check_stage_free(pdhg_handle *h) {
  BatchState::Checks &C = h->bat->chk;
  if (C.upload_pending) {
    HIP_TRY(hipEventSynchronize(C.uploaded));
    C.upload_pending = false;
  }
  memset(C.stage_host->out, 0, sizeof(C.stage_host->out));
  return 0;
}

// The upload and the passes of a call: per pass the pack kernel, then per matrix one batched product -- or, where the
// batch's product has long rows, each masked member's own.  `carried` entries of S.ev travel with the same upload.
static int batch_check_passes(pdhg_handle *h, BatchCheckCall &call, CheckMarks &marks) {
  BatchState &B = *h->bat;
  BatchState::Checks &C = B.chk;
  BatchCheckStage &S = *C.stage_host;
  const int n = (int)h->n, m = (int)h->m;
  const bool qp = h->has_q;
  // which products ride a batched launch (all rows within the row order's sequential limit: the member's own order)
  const bool bA = m > 0 && B.PA.nlong == 0, bT = n > 0 && m > 0 && B.PT.nlong == 0, bQ = qp && B.PQ.nlong == 0;
  const bool oA = m > 0 && !bA, oT = n > 0 && !bT, oQ = qp && !bQ;
  bool launch_pack[3];
  for (int p = 0; p < 3; ++p) {
    launch_pack[p] = false;
    for (int s = 0; s < call.count[p]; ++s) {
      if (!(bA || bT || bQ)) S.pts[p][s].pack = 0;
      launch_pack[p] = launch_pack[p] || S.pts[p][s].pack || S.pts[p][s].do_div;
    }
  }
  HIP_TRY(hipMemcpyAsync(C.stage_dev, C.stage_host, sizeof(BatchCheckStage), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipEventRecord(C.uploaded, h->stream));
  C.upload_pending = true;
  int rc;
  for (int p = 0; p < 3; ++p) {
    if (launch_pack[p]) {
      hipLaunchKernelGGL(batch_check_pack_kernel, dim3(ew_grid(std::max(n, m)), call.count[p]), dim3(TPB), 0, h->stream, n, m,
                         (const BatchCheckPoint *)C.stage_dev->pts[p], B.X, B.Y, B.shift);
      HIP_TRY(hipGetLastError());
      C.launches += 1;
    }
    const unsigned mask = call.mask[p];
    if (!mask) continue;
    const int items = __builtin_popcount(mask);
    if (bA || bT || bQ) C.batched += items;
    if (oA || oT || oQ) C.own += items;
    auto batched = [&](const CsrDev &D, BatchProduct &P, const double *gather, int which) {
      BatchArgs a{B.mdev, B.act_dev, mask, B.K, B.shift, const_cast<double *>(gather), B.Y};
      hipLaunchKernelGGL((batch_spmv_kernel<MODE_PLAIN, double *const *>), dim3(P.grid), dim3(TPB), 0, h->stream, P.rows, D.rowptr,
                         D.col, D.val, P.long_thr, a, P.part, P.slots, (double *const *)C.stage_dev->out[p][which]);
      C.launches += 1;
    };
    if (bA) batched(h->A, B.PA, B.X, 0);
    if (bT) batched(h->At, B.PT, B.Y, 1);
    if (bQ) batched(h->Q, B.PQ, B.X, 2);
    HIP_TRY(hipGetLastError());
    if (!(oA || oT || oQ)) continue;
    for (int k = 0; k < B.K; ++k) {
      if (!((mask >> k) & 1u)) continue;
      pdhg_handle *mb = B.mem[(size_t)k];
      const PointRef &pt = call.pt[p][k];
      EpiArgs e{};
      if (oA) { e.out = pt.ax; if ((rc = launch_spmv<MODE_PLAIN, 0>(mb, mb->A, pt.px, e))) return rc; C.launches += 1; }
      if (oT) { if ((rc = launch_aty_plain(mb, pt.py, pt.aty))) return rc; C.launches += 1; }
      if (oQ) { e.out = pt.qx; if ((rc = launch_spmv<MODE_PLAIN, 2>(mb, mb->Q, pt.px, e))) return rc; C.launches += 1; }
    }
  }
  marks.issued = true;
  return 0;
}

static int batch_checks_begin(pdhg_handle *batch, const char *who) {
  if (!batch) return fail(-1, std::string(who) + ": null handle");
  if (!batch_of(batch)) return fail(-1, std::string(who) + ": not a batch handle");
  return 0;
}

// what is pending on the members a call touches is settled first; their evaluation buffers exist
static int batch_check_settle(pdhg_handle *h, unsigned members) {
  int rc;
  for (int k = 0; k < h->bat->K; ++k) {
    if (!((members >> k) & 1u)) continue;
    pdhg_handle *m = h->bat->mem[(size_t)k];
    { Shards L = shards_of(m); if ((rc = flush_pending(L))) return rc; }
    if ((rc = ev_alloc(m))) return rc;
  }
  return 0;
}

/* A x, A' y (and Q x) at point[i] of member[i], i < count, into the members' per-point caches (pdhg_hip_batch_checks.h). */
int pdhg_batch_point_products(pdhg_handle *batch, int count, const int *member, const int *point) {
  RoctxRange roctx_range("pdhg_batch_point_products");
  int rc = batch_checks_begin(batch, "pdhg_batch_point_products");
  if (rc) return rc;
  if ((rc = batch_awaits_rescale(batch, "pdhg_batch_point_products: "))) return rc;
  if (count < 1 || count > 3 * BATCH_MAX) return fail(-1, "pdhg_batch_point_products: count must be 1.." + std::to_string(3 * BATCH_MAX));
  if (!member || !point) return fail(-1, "null argument");
  pdhg_handle *h = batch;
  unsigned members = 0;
  for (int i = 0; i < count; ++i) {
    if ((rc = batch_check_refuse(h, member[i], point[i], "pdhg_batch_point_products: item " + std::to_string(i)))) return rc;
    members |= 1u << member[i];
  }
  HIP_TRY(hipSetDevice(h->device));
  if ((rc = batch_checks_ensure(h))) return rc;
  if ((rc = batch_check_settle(h, members))) return rc;
  if ((rc = batch_check_stage_free(h))) return rc;
  BatchState::Checks &C = h->bat->chk;
  C.calls += 1;
  BatchCheckCall call;
  CheckMarks marks;
  for (int i = 0; i < count; ++i) {
    PointClaim pt;
    if ((rc = batch_check_stage(h, member[i], point[i], true, *C.stage_host, call, marks, &pt))) return rc;
    if (!pt.stale) C.cached += 1;
  }
  if (!(call.count[0] | call.count[1] | call.count[2])) { marks.issued = true; return 0; }
  return batch_check_passes(h, call, marks);
}

/* pdhg_eval_point(member k, points[k], out + 24 k) for every k with points[k] >= 0 (pdhg_hip_batch_checks.h). */
int pdhg_batch_eval_points(pdhg_handle *batch, const int *points, double *out) {
  RoctxRange roctx_range("pdhg_batch_eval_points");
  int rc = batch_checks_begin(batch, "pdhg_batch_eval_points");
  if (rc) return rc;
  if ((rc = batch_awaits_rescale(batch, "pdhg_batch_eval_points: "))) return rc;
  if (!points || !out) return fail(-1, "null argument");
  pdhg_handle *h = batch;
  BatchState &B = *h->bat;
  unsigned members = 0;
  for (int k = 0; k < B.K; ++k) {
    if (points[k] < 0) continue;
    const std::string who = "pdhg_batch_eval_points: member " + std::to_string(k);
    if ((rc = batch_check_refuse(h, k, points[k], who))) return rc;
    if (!B.mem[(size_t)k]->has_original) return fail(-1, who + ": pdhg_set_original_problem has not been called");
    members |= 1u << k;
  }
  HIP_TRY(hipSetDevice(h->device));
  h->bchk_asked = true;
  BatchState::Checks &C = B.chk;
  C.calls += 1;
  if (!members) return 0;
  // without the form the kernels here restate, or with a profiled member, every member is served by its own call inside this one
  bool shared = eval_shared_form_in_force();
  for (int k = 0; k < B.K; ++k) if (((members >> k) & 1u) && B.mem[(size_t)k]->profile) shared = false;
  if (!shared) {
    for (int k = 0; k < B.K; ++k)
      if (((members >> k) & 1u) && (rc = serve_eval_by_own_call(h->bchk_serving, B.mem[(size_t)k], points[k], out + (size_t)24 * k)))
        return rc;
    return 0;
  }
  if ((rc = batch_checks_ensure(h))) return rc;
  if ((rc = batch_check_settle(h, members))) return rc;
  if ((rc = batch_check_stage_free(h))) return rc;
  BatchCheckStage &S = *C.stage_host;
  BatchCheckCall call;
  CheckMarks marks;
  struct Carried { int k; bool have_avg; };
  std::vector<Carried> carried;
  const unsigned long long seq = ++C.seq;
  const size_t words = (size_t)(EV_HOST_SLOTS + 2);
  for (int k = 0; k < B.K; ++k) {
    if (!((members >> k) & 1u)) continue;
    pdhg_handle *m = B.mem[(size_t)k];
    PointClaim pt, av;
    if ((rc = batch_check_stage(h, k, points[k], true, S, call, marks, &pt))) return rc;
    if (!pt.stale) C.cached += 1;
    const bool have_avg = m->sum_x_count != 0 && m->sum_y_count != 0;
    if (have_avg && (rc = batch_check_stage(h, k, PDHG_POINT_AVERAGE, false, S, call, marks, &av))) return rc;
    S.ev[carried.size()] = eval_args_of(m, pt, have_avg, C.res + carried.size() * words, seq);
    carried.push_back(Carried{k, have_avg});
  }
  C.carried += (int64_t)carried.size();
  if ((rc = batch_check_passes(h, call, marks))) return rc;
  // every member of a batch has one n and m: one ev_grid, the launches' x extent
  const int G = B.mem[(size_t)carried[0].k]->ev_grid;
  const unsigned nc = (unsigned)carried.size();
  const FleetQpEvalArgs *table = C.stage_dev->ev;
  hipLaunchKernelGGL(batch_eval_rows_kernel, dim3(G, nc), dim3(TPB), 0, h->stream, table);
  hipLaunchKernelGGL(batch_eval_cols_kernel, dim3(G, nc), dim3(TPB), 0, h->stream, table);
  hipLaunchKernelGGL(batch_eval_dist_kernel, dim3(G, nc, 3), dim3(TPB), 0, h->stream, table);
  hipLaunchKernelGGL(batch_eval_final_kernel, dim3(nc), dim3(FINAL_TPB), 0, h->stream, table);
  HIP_TRY(hipGetLastError());
  C.launches += 4;
  for (size_t j = 0; j < carried.size(); ++j) {
    const int k = carried[j].k;
    pdhg_handle *m = B.mem[(size_t)k];
    double r[28];
    if ((rc = wait_words(h->stream, C.res + j * words, EV_HOST_SLOTS, 28, seq, r, 40000000L,
                         "a batch's evaluation launch finished without publishing its results")))
      return rc;
    double *o = out + (size_t)24 * k;
    eval_unpack(m, points[k], true, carried[j].have_avg, r, o);
    fleet_store_eval(m, points[k], o);
  }
  return 0;
}

/* out[0..7]: what the two calls above and the members' own evaluations did so far (pdhg_hip_batch_checks.h). */
int pdhg_batch_check_info(pdhg_handle *batch, int64_t out[8]) {
  if (!out) return fail(-1, "out == NULL");
  int rc = batch_checks_begin(batch, "pdhg_batch_check_info");
  if (rc) return rc;
  const BatchState::Checks &C = batch->bat->chk;
  out[0] = C.calls; out[1] = C.batched; out[2] = C.own; out[3] = C.cached; out[4] = C.carried;
  out[5] = batch->bchk_served; out[6] = batch->bchk_misses; out[7] = C.launches;
  return 0;
}
