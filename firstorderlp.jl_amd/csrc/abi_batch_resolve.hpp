// abi_batch_resolve.hpp -- part of the single translation unit pdhg_hip.hip (included there, inside its extern "C" block, last).
// C ABI: RE-SOLVES of a batch on its handle (include/pdhg_hip_batch_resolve.h; kernels in batch_resolve_kernels.hpp).
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
  return 0;
}

static double *batch_resolve_data(double *stage) { return (double *)((char *)stage + BATCH_RESOLVE_HEAD_BYTES); }

int pdhg_batch_resolve_retain(pdhg_handle *batch) {
  int rc = batch_resolve_refuse(batch, "pdhg_batch_resolve_retain", false);
  if (rc) return rc;
  pdhg_handle *h = batch;
  if (h->rs) return 0;
  if ((rc = check_handle(h, true, true))) return rc;
  const int64_t n = h->n, m = h->m;
  const int64_t len = (int64_t)(BATCH_RESOLVE_HEAD_BYTES / sizeof(double)) + (int64_t)h->bat->K * (3 * n + m);
  ResolveState *R = new ResolveState();
  h->rs = R;
  auto body = [&]() -> int {
    int r2;
    if ((r2 = alloc_zero(&R->cum_d, n))) return r2;
    if ((r2 = alloc_zero(&R->cum_e, m))) return r2;
    if ((r2 = alloc_zero(&R->stage_dev, len))) return r2;
    HIP_TRY(hipHostMalloc((void **)&R->stage_host, sizeof(double) * (size_t)len, hipHostMallocDefault));
    hipLaunchKernelGGL(fill_kernel, dim3(h->ew_grid_n), dim3(TPB), 0, h->stream, (int)n, 1.0, R->cum_d);
    hipLaunchKernelGGL(fill_kernel, dim3(h->ew_grid_m), dim3(TPB), 0, h->stream, (int)m, 1.0, R->cum_e);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
  };
  rc = body();
  if (rc) resolve_release(h);
  return rc;
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
  B.rsv_carried = (int64_t)carried.size();
  B.rsv_single = 0;
  if (carried.empty()) return 0;
  if ((rc = check_handle(h, true, true))) return rc;
  for (int k : carried) {          // a pending lazy accept belongs to the iterate, not to these four arrays: settled
    Shards L = shards_of(B.mem[(size_t)k]);
    if ((rc = flush_pending(L))) return rc;
  }
  BatchReplayMember *table = (BatchReplayMember *)R.stage_host;
  double *data_host = batch_resolve_data(R.stage_host);
  const double *data_dev = batch_resolve_data(R.stage_dev);
  size_t off = 0, placed = 0;
  auto put = [&](const double *src, int64_t len) -> const double * {
    if (!src) return nullptr;
    if (len > 0) memcpy(data_host + off, src, sizeof(double) * (size_t)len);
    const double *at = data_dev + off;
    off += (size_t)len;
    return at;
  };
  for (int k : carried) {
    pdhg_handle *mb = B.mem[(size_t)k];
    BatchReplayMember e{};
    e.in_c = put(resolve_entry(c, k), h->n); e.in_lb = put(resolve_entry(lb, k), h->n);
    e.in_ub = put(resolve_entry(ub, k), h->n); e.in_b = put(resolve_entry(b, k), h->m);
    e.c = mb->c; e.lb = mb->lb; e.ub = mb->ub; e.b = mb->b;
    table[placed++] = e;
  }
  const int tiles = (int)((placed + BATCH_RESOLVE_TILE - 1) / BATCH_RESOLVE_TILE);
  while (placed < (size_t)tiles * BATCH_RESOLVE_TILE) table[placed++] = BatchReplayMember{};      // the last tile's tail: nothing
  HIP_TRY(hipMemcpyAsync(R.stage_dev, R.stage_host, BATCH_RESOLVE_HEAD_BYTES + sizeof(double) * off, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(batch_resolve_replay_kernel, dim3(h->ew_grid_nm, tiles), dim3(TPB), 0, h->stream, (int)h->n, (int)h->m,
                     (int)R.steps, (const double *)R.rec, (const BatchReplayMember *)R.stage_dev);
  HIP_TRY(hipGetLastError());
  B.rsv_launches += 1;
  for (int k : carried) {
    pdhg_handle *mb = B.mem[(size_t)k];
    mb->state_version += 1;
    fleet_forget(mb);
    // K view rebuilds -- each a synchronisation and an allocation -- would undo the shared launch: the views are rebuilt
    // where they are next read (bounds_fresh); the batched primal kernel reads the dense arrays and never needs them
    if (resolve_entry(lb, k) || resolve_entry(ub, k)) mb->bnd_dirty = true;
  }
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
  B.rsv_carried = (int64_t)carried.size();
  B.rsv_single = 0;
  B.rsv_batched = 0;
  if (carried.empty()) return 0;
  if ((rc = check_handle(h, true, true))) return rc;
  // Every row of A' inside the row order's sequential limit: the batched row sum -- one lane, left to right from 0.0 -- is
  // the member's own product bit for bit.  With long rows present the members take their own products.
  const bool batched = B.PT.nlong == 0 && h->n > 0 && h->m > 0;
  BatchPointMember *table = (BatchPointMember *)R.stage_host;
  double **aty_host = (double **)((char *)R.stage_host + BATCH_RESOLVE_TABLE_BYTES);
  double *const *aty_dev = (double *const *)((char *)R.stage_dev + BATCH_RESOLVE_TABLE_BYTES);
  double *data_host = batch_resolve_data(R.stage_host);
  const double *data_dev = batch_resolve_data(R.stage_dev);
  size_t off = 0, placed = 0;
  unsigned mask = 0;
  std::vector<int> own;
  for (int k = 0; k < BATCH_MAX; ++k) aty_host[k] = k < B.K ? B.mem[(size_t)k]->aty : nullptr;
  for (int k : carried) {
    pdhg_handle *mb = B.mem[(size_t)k];
    const double *px = resolve_entry(x, k), *py = resolve_entry(y, k);
    resolve_clear_host(mb);
    BatchPointMember e{};
    if (px) { if (h->n > 0) memcpy(data_host + off, px, sizeof(double) * (size_t)h->n); e.in_x = data_dev + off; off += (size_t)h->n; }
    if (py) { if (h->m > 0) memcpy(data_host + off, py, sizeof(double) * (size_t)h->m); e.in_y = data_dev + off; off += (size_t)h->m; }
    e.x = mb->x; e.y = mb->y; e.aty = mb->aty;
    e.zn[0] = mb->sum_x; e.zn[1] = mb->sum_x_alt; e.zn[2] = mb->x_r; e.zn[3] = mb->has_q ? mb->qx : nullptr; e.zn[4] = mb->has_q ? mb->qx2 : nullptr;
    e.zm[0] = mb->sum_y; e.zm[1] = mb->sum_y_alt; e.zm[2] = mb->y_r;
    e.zero_aty = py ? 0 : 1;
    e.pack_k = -1;
    if (py && batched) { e.pack_k = k; mask |= 1u << k; }
    else if (py) own.push_back(k);
    table[placed++] = e;
  }
  HIP_TRY(hipMemcpyAsync(R.stage_dev, R.stage_host, BATCH_RESOLVE_HEAD_BYTES + sizeof(double) * off, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(batch_resolve_point_kernel, dim3(h->ew_grid_nm, (unsigned)placed), dim3(TPB), 0, h->stream, (int)h->n, (int)h->m,
                     (const double *)(R.steps > 0 ? R.cum_d : nullptr), (const double *)(R.steps > 0 ? R.cum_e : nullptr),
                     (const BatchPointMember *)R.stage_dev, B.Y, B.shift);
  HIP_TRY(hipGetLastError());
  B.rsv_launches += 1;
  if (mask) {
    // A' Y of the masked members row by row into their A'y: the product a QP batch runs for Q X, gathering from Y
    BatchArgs a{B.mdev, B.act_dev, mask, B.K, B.shift, B.Y, B.Y};
    BatchProduct &P = B.PT;
    hipLaunchKernelGGL((batch_spmv_kernel<MODE_PLAIN, double *const *>), dim3(P.grid), dim3(TPB), 0, h->stream, P.rows,
                       h->At.rowptr, h->At.col, h->At.val, P.long_thr, a, P.part, P.slots, aty_dev);
    HIP_TRY(hipGetLastError());
    B.rsv_launches += 1;
    B.rsv_batched = 1;
  }
  B.rsv_single = (int64_t)own.size();
  for (int k : own) {
    Shards L = shards_of(B.mem[(size_t)k]);
    if ((rc = dual_product(L, [](pdhg_handle *s) { return (const double *)s->y; }, [](pdhg_handle *s) { return s->aty; }))) return rc;
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

int pdhg_batch_resolve_info(pdhg_handle *batch, int64_t out[4]) {
  if (!out) return fail(-1, "out == NULL");
  int rc = batch_resolve_refuse(batch, "pdhg_batch_resolve_info", false);
  if (rc) return rc;
  const BatchState &B = *batch->bat;
  out[0] = B.rsv_launches; out[1] = B.rsv_carried; out[2] = B.rsv_single; out[3] = B.rsv_batched;
  return 0;
}
