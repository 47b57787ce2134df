// abi_batch_resolve.hpp -- part of the single translation unit pdhg_hip.hip (included there, inside its extern "C" block, last).
// C ABI: RE-SOLVES of a batch on its handle (include/pdhg_hip_batch_resolve.h; kernels in batch_resolve_kernels.hpp;
// what this form shares with a single handle's and a fleet's, abi_resolve.hpp, in host_resolve.hpp).
// A batch's members share the matrix, so create, the layouts and every rescaling pass depend on nothing a tick changes:
//
//   pdhg_batch_resolve_retain            before pdhg_rescale on the batch handle: ONE ResolveState on the batch handle --
//                                        apply_scaling records each step there before it scales the members' vectors
//   pdhg_batch_update_problem_vectors    one packed upload, ONE launch that replays the record on every carried member
//   pdhg_batch_warm_start                one upload, one launch for the points; A'y of the members given a y in one
//                                        batched product where that is the member's own product bit for bit
//   pdhg_batch_resolve_info              what the last call did
//
// The staging buffers (ResolveState::stage_host / stage_dev) begin with a head -- the call's member table and the table
// of the members' A'y -- and hold K (3 n + m) doubles behind it.

static int batch_resolve_refuse(pdhg_handle *b, const std::string &who, bool need_record) {
  if (!b) return fail(-1, who + ": null handle");
  if (!batch_of(b)) return fail(-1, who + ": not a batch handle");
  if (need_record && !b->rs) return fail(-1, who + ": pdhg_batch_resolve_retain was not called on this batch before pdhg_rescale");
  if (need_record) return batch_awaits_rescale(b, who + ": ");       // (given new matrix values and not rescaled since)
  return 0;
}

static double *batch_resolve_data(double *stage) { return (double *)((char *)stage + BATCH_RESOLVE_HEAD_BYTES); }

int pdhg_batch_resolve_retain(pdhg_handle *batch) {
  const int rc = batch_resolve_refuse(batch, "pdhg_batch_resolve_retain", false);
  return rc ? rc : resolve_retain(batch, (int64_t)(BATCH_RESOLVE_HEAD_BYTES / sizeof(double)) + (int64_t)batch->bat->K * (3 * batch->n + batch->m));
}

int pdhg_batch_update_problem_vectors(pdhg_handle *batch, const double *const *c, const double *const *b,
                                      const double *const *lb, const double *const *ub) {
  RoctxRange roctx_range("pdhg_batch_update_problem_vectors");
  int rc = batch_resolve_refuse(batch, "pdhg_batch_update_problem_vectors", true);
  if (rc) return rc;
  pdhg_handle *h = batch;
  BatchState &B = *h->bat;
  ResolveState &R = *h->rs;
  std::vector<int> carried;
  for (int k = 0; k < B.K; ++k)
    if (resolve_entry(c, k) || resolve_entry(b, k) || resolve_entry(lb, k) || resolve_entry(ub, k)) carried.push_back(k);
  B.rsv.carried = (int64_t)carried.size();
  B.rsv.single = 0;
  if (carried.empty()) return 0;
  if ((rc = check_handle(h, true, true))) return rc;
  for (int k : carried) {          // a pending lazy accept belongs to the iterate, not to these four arrays: settled
    Shards L = shards_of(B.mem[(size_t)k]);
    if ((rc = flush_pending(L))) return rc;
  }
  ResolveReplayMember *table = (ResolveReplayMember *)R.stage_host;
  ResolveStage S{batch_resolve_data(R.stage_host), batch_resolve_data(R.stage_dev)};
  size_t placed = 0;
  for (int k : carried)
    table[placed++] = resolve_replay_member(B.mem[(size_t)k], S, resolve_entry(c, k), resolve_entry(b, k), resolve_entry(lb, k), resolve_entry(ub, k));
  const int tiles = (int)((placed + BATCH_RESOLVE_TILE - 1) / BATCH_RESOLVE_TILE);
  while (placed < (size_t)tiles * BATCH_RESOLVE_TILE) table[placed++] = ResolveReplayMember{};      // the last tile's tail: nothing
  HIP_TRY(hipMemcpyAsync(R.stage_dev, R.stage_host, BATCH_RESOLVE_HEAD_BYTES + sizeof(double) * S.off, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(batch_resolve_replay_kernel, dim3(h->ew_grid_nm, tiles), dim3(TPB), 0, h->stream, (int)h->n, (int)h->m,
                     (int)R.steps, (const double *)R.rec, (const ResolveReplayMember *)R.stage_dev);
  HIP_TRY(hipGetLastError());
  B.rsv.launches += 1;
  for (int k : carried) resolve_member_updated(B.mem[(size_t)k], resolve_entry(lb, k) || resolve_entry(ub, k));
  HIP_TRY(hipStreamSynchronize(h->stream));              // (the staging buffer is free for the next call)
  return 0;
}

int pdhg_batch_warm_start(pdhg_handle *batch, const double *const *x, const double *const *y) {
  RoctxRange roctx_range("pdhg_batch_warm_start");
  int rc = batch_resolve_refuse(batch, "pdhg_batch_warm_start", true);
  if (rc) return rc;
  pdhg_handle *h = batch;
  BatchState &B = *h->bat;
  ResolveState &R = *h->rs;
  const bool everyone = !x && !y;               // NULL arrays: zeros for every member; a member with two NULL entries is left alone
  std::vector<int> carried;
  for (int k = 0; k < B.K; ++k)
    if (everyone || resolve_entry(x, k) || resolve_entry(y, k)) carried.push_back(k);
  B.rsv.carried = (int64_t)carried.size();
  B.rsv.single = 0;
  B.rsv.other = 0;
  if (carried.empty()) return 0;
  if ((rc = check_handle(h, true, true))) return rc;
  // Every row of A' inside the row order's sequential limit: the batched row sum -- one lane, left to right from 0.0 -- is
  // the member's own product bit for bit.  With long rows present the members take their own products.
  const bool batched = B.PT.nlong == 0 && h->n > 0 && h->m > 0;
  BatchPointMember *table = (BatchPointMember *)R.stage_host;
  double **aty_host = (double **)((char *)R.stage_host + BATCH_RESOLVE_TABLE_BYTES);
  double *const *aty_dev = (double *const *)((char *)R.stage_dev + BATCH_RESOLVE_TABLE_BYTES);
  ResolveStage S{batch_resolve_data(R.stage_host), batch_resolve_data(R.stage_dev)};
  size_t placed = 0;
  unsigned mask = 0;
  std::vector<int> own;
  for (int k = 0; k < BATCH_MAX; ++k) aty_host[k] = k < B.K ? B.mem[(size_t)k]->aty : nullptr;
  for (int k : carried) {
    pdhg_handle *mb = B.mem[(size_t)k];
    const double *px = resolve_entry(x, k), *py = resolve_entry(y, k);
    resolve_clear_host(mb);
    BatchPointMember e{};
    e.in_x = S.put(px, h->n); e.in_y = S.put(py, h->m);
    e.x = mb->x; e.y = mb->y; e.aty = mb->aty;
    e.z = resolve_fresh_zeros(mb);
    e.zero_aty = py ? 0 : 1;
    e.pack_k = -1;
    if (py && batched) { e.pack_k = k; mask |= 1u << k; }
    else if (py) own.push_back(k);
    table[placed++] = e;
  }
  HIP_TRY(hipMemcpyAsync(R.stage_dev, R.stage_host, BATCH_RESOLVE_HEAD_BYTES + sizeof(double) * S.off, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(batch_resolve_point_kernel, dim3(h->ew_grid_nm, (unsigned)placed), dim3(TPB), 0, h->stream, (int)h->n, (int)h->m,
                     (const double *)(R.steps > 0 ? R.cum_d : nullptr), (const double *)(R.steps > 0 ? R.cum_e : nullptr),
                     (const BatchPointMember *)R.stage_dev, B.Y, B.shift);
  HIP_TRY(hipGetLastError());
  B.rsv.launches += 1;
  if (mask) {
    // A' Y of the masked members row by row into their A'y: the product a QP batch runs for Q X, gathering from Y
    BatchArgs a{B.mdev, B.act_dev, mask, B.K, B.shift, B.Y, B.Y};
    BatchProduct &P = B.PT;
    hipLaunchKernelGGL((batch_spmv_kernel<MODE_PLAIN, double *const *>), dim3(P.grid), dim3(TPB), 0, h->stream, P.rows,
                       h->At.rowptr, h->At.col, h->At.val, P.long_thr, a, P.part, P.slots, aty_dev);
    HIP_TRY(hipGetLastError());
    B.rsv.launches += 1;
    B.rsv.other = 1;
  }
  B.rsv.single = (int64_t)own.size();
  for (int k : own)
    if ((rc = resolve_own_aty(B.mem[(size_t)k]))) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

int pdhg_batch_resolve_info(pdhg_handle *batch, int64_t out[4]) {
  if (!out) return fail(-1, "out == NULL");
  int rc = batch_resolve_refuse(batch, "pdhg_batch_resolve_info", false);
  if (rc) return rc;
  resolve_info(batch->bat->rsv, out);
  return 0;
}
