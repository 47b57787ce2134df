// abi_batch_matrix_update.hpp -- part of the single translation unit pdhg_hip.hip (included there, inside its extern "C" block, last).
// C ABI: NEW MATRIX VALUES for a BATCH whose sparsity pattern is kept (include/pdhg_hip_batch_matrix_update.h).  No kernel
// of its own: the placement is abi_matrix_update.hpp's on the batch handle's layouts (the members' are struct copies of
// the same device arrays), the members' vectors come back through abi_batch_resolve.hpp's replay launch.
//
//   pdhg_batch_update_matrix_values   values into every copy of A, A', Q, Q'; member 0's raw vectors into the batch handle's
//                                     own; the record reset; ALL members' raw vectors staged on the device behind their
//                                     replay table; the batch marked pdhg_handle::members_await_rescale
//   pdhg_rescale on the marked batch  (abi_rescale.hpp) records its steps, skips batch_scale_members -- K launches and K
//                                     syncing view rebuilds per step -- and ends in batch_replay_staged_members below:
//                                     one batch_resolve_replay_kernel launch over all K members, then the mark is cleared
//
// Between the two calls nothing else runs on the batch or its members (batch_awaits_rescale), so the staging buffer --
// exactly the head and K (3 n + m) doubles -- keeps the table and the vectors from the one call to the other.

// the end of pdhg_rescale on a batch whose members await it; the stream is synchronised by that call
static int batch_replay_staged_members(pdhg_handle *h) {
  BatchState &B = *h->bat;
  ResolveState &R = *h->rs;
  const int tiles = (B.K + BATCH_RESOLVE_TILE - 1) / BATCH_RESOLVE_TILE;
  // (a record of zero steps: the staged raw vectors are copied)
  hipLaunchKernelGGL(batch_resolve_replay_kernel, dim3(h->ew_grid_nm, tiles), dim3(TPB), 0, h->stream, (int)h->n, (int)h->m,
                     (int)R.steps, (const double *)R.rec, (const ResolveReplayMember *)R.stage_dev);
  HIP_TRY(hipGetLastError());
  B.rsv.launches += 1;
  B.rsv.carried = B.K;
  B.rsv.single = 0;
  for (pdhg_handle *m : B.mem) {
    resolve_member_updated(m, true);       // (the bound views: rebuilt where they are next read, as after a vector update)
    m->matrix_version += 1;                // the shared matrix was scaled under the member
  }
  h->members_await_rescale = 0;
  return 0;
}

int pdhg_batch_update_matrix_values(pdhg_handle *batch, int64_t nnz, const double *nzval, int64_t q_nnz, const double *q_nzval,
                                    const double *const *c, const double *const *b, const double *const *lb,
                                    const double *const *ub) {
  RoctxRange roctx_range("pdhg_batch_update_matrix_values");
  const std::string who = "pdhg_batch_update_matrix_values";
  // every refusal first: nothing is launched, settled or written when one is reported
  int rc = batch_resolve_refuse(batch, who, true);
  if (rc) return rc;
  pdhg_handle *h = batch;
  BatchState &B = *h->bat;
  if (nnz != h->nnz)
    return fail(-1, who + ": nnz = " + std::to_string(nnz) + ", the batch was created with " + std::to_string(h->nnz) + " (the pattern is kept)");
  if (!nzval) return fail(-1, who + ": nzval == NULL");
  if (!c || !b || !lb || !ub) return fail(-1, who + ": the tables c, b, lb and ub are all needed (the batch is rescaled afterwards: they hold the raw vectors)");
  for (int k = 0; k < B.K; ++k)
    if ((h->n > 0 && (!c[k] || !lb[k] || !ub[k])) || (h->m > 0 && !b[k]))
      return fail(-1, who + ": member " + std::to_string(k) + ": c, b, lb and ub are all needed (a NULL table entry)");
  if (!h->has_q && (q_nnz != 0 || q_nzval)) return fail(-1, who + ": q_nzval on an LP batch (an update cannot turn an LP into a QP)");
  if (h->has_q && !q_nzval) return fail(-1, who + ": the batch has an objective matrix: q_nzval == NULL");
  if (h->has_q && q_nnz != h->Q.nnz)
    return fail(-1, who + ": q_nnz = " + std::to_string(q_nnz) + ", the objective matrix was set with " + std::to_string(h->Q.nnz));
  if ((rc = check_handle(h, true, true))) return rc;
  // (the one refusal that needs the device, and only on a batch's first update: a read-only pass)
  if ((rc = mu_pattern_ascending(h))) return rc;
  if (!h->csc_ascending)
    return fail(-1, who + ": the batch was created from columns whose row indices do not ascend strictly (unsorted or duplicate "
                          "entries): their values cannot be placed by search; create a new batch");
  for (pdhg_handle *m : B.mem) {             // a pending lazy accept belongs to the iterate: settled before the versions move
    Shards L = shards_of(m);
    if ((rc = flush_pending(L))) return rc;
  }

  ResolveState &R = *h->rs;
  MuSourceHost from_at, from_qt;
  auto body = [&]() -> int {
    int r2;
    if ((r2 = mu_upload_values(h, h->At, nzval))) return r2;
    if ((r2 = mu_source(h->At, from_at))) return r2;
    place_matrix_values(h, h->At, nullptr);
    place_matrix_values(h, h->A, &from_at.src);
    if (h->has_q) {
      if ((r2 = mu_upload_values(h, h->Qt, q_nzval))) return r2;
      if ((r2 = mu_source(h->Qt, from_qt))) return r2;
      place_matrix_values(h, h->Qt, nullptr);
      place_matrix_values(h, h->Q, &from_qt.src);
    }
    HIP_TRY(hipGetLastError());
    // the batch handle's own vectors: member 0's raw ones, as pdhg_create_batch uploads them
    const struct { double *dst; const double *src; int64_t len; } vec[4] = {{h->c, c[0], h->n}, {h->b, b[0], h->m}, {h->lb, lb[0], h->n}, {h->ub, ub[0], h->n}};
    for (const auto &v : vec)
      if (v.len > 0) HIP_TRY(hipMemcpyAsync(v.dst, v.src, sizeof(double) * (size_t)v.len, hipMemcpyHostToDevice, h->stream));
    // the retained record starts again (its capacity stays: the pdhg_rescale that follows reuses it)
    R.steps = 0;
    hipLaunchKernelGGL(fill_kernel, dim3(h->ew_grid_n), dim3(TPB), 0, h->stream, (int)h->n, 1.0, R.cum_d);
    hipLaunchKernelGGL(fill_kernel, dim3(h->ew_grid_m), dim3(TPB), 0, h->stream, (int)h->m, 1.0, R.cum_e);
    HIP_TRY(hipGetLastError());
    // every member's four raw vectors behind the replay table, uploaded now: the staging buffers hold exactly these
    ResolveReplayMember *table = (ResolveReplayMember *)R.stage_host;
    ResolveStage S{batch_resolve_data(R.stage_host), batch_resolve_data(R.stage_dev)};
    size_t placed = 0;
    for (int k = 0; k < B.K; ++k) table[placed++] = resolve_replay_member(B.mem[(size_t)k], S, c[k], b[k], lb[k], ub[k]);
    const size_t tiles = (placed + BATCH_RESOLVE_TILE - 1) / BATCH_RESOLVE_TILE;
    while (placed < tiles * BATCH_RESOLVE_TILE) table[placed++] = ResolveReplayMember{};      // the last tile's tail: nothing
    HIP_TRY(hipMemcpyAsync(R.stage_dev, R.stage_host, BATCH_RESOLVE_HEAD_BYTES + sizeof(double) * S.off, hipMemcpyHostToDevice, h->stream));
    return 0;
  };
  rc = body();
  // The evaluation caches, the members' per-point products and their stored check results are keyed by these versions.
  // BatchProduct, X, Y and DX hold indices and scratch only.  The members' points, sums and restart points are left as
  // they are: they belong to the old scaling, and the warm start every solve begins with empties them.
  h->state_version += 1;
  h->matrix_version += 1;
  for (pdhg_handle *m : B.mem) {
    m->state_version += 1;
    m->matrix_version += 1;
    fleet_forget(m);
  }
  // A device error after the first placement was queued leaves new raw values under vectors of the old scaling: nothing
  // but pdhg_destroy proceeds on such a batch (2).
  h->members_await_rescale = rc ? 2 : 1;
  // lb / ub of the batch handle are raw again, and a record of zero steps runs no apply_scaling that would rebuild their views
  const int rcb = bounds_rebuild(h);                    // (returns with the stream idle)
  if (rcb) (void)hipStreamSynchronize(h->stream);
  for (MuPiece *p : {from_at.dev, from_qt.dev}) if (p) (void)hipFree(p);
  return rc ? rc : rcb;
}
