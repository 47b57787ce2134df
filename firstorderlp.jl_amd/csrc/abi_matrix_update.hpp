// abi_matrix_update.hpp -- part of the single translation unit pdhg_hip.hip (included there, inside its extern "C" block, last).
// C ABI: NEW MATRIX VALUES on a live handle whose sparsity pattern is kept (include/pdhg_hip_matrix_update.h; kernels in
// matrix_update_kernels.hpp).  Layout construction, the host builders, the create-time timing of sweep variants and every
// allocation depend on the pattern only: a caller whose A (and Q) get new entries in the same places keeps the handle,
// sends the new values in the order of the create call, and rescales again.
//
// What is placed from what:
//   CSR(A').val                 the caller's array as it is (CSR(A') is the CSC narrowed to 32 bits), segment by segment
//   CSR(A).val                  entry (i, j) from row j of CSR(A'), by binary search for i
//   sweep copy, column slabs    entry (i, j) from row i of the SAME matrix's refreshed CSR, by binary search for j
//   sliced jagged copies        sj_fill_kernel from the refreshed CSR arrays, as apply_scaling refills them
// and the same for Q' / Q.  Nothing per nonzero stays on the handle: the searches are a few dependent loads per entry,
// once per update.

// the searched matrix as the kernels take it; `dev` (a table of row segments) is the caller's to free once the stream is idle
struct MuSourceHost {
  MuSource src{};
  MuPiece *dev = nullptr;
};
static int mu_source(const CsrDev &T, MuSourceHost &out) {
  if (T.segs.empty()) {
    out.src = MuSource{1, nullptr, MuPiece{0, T.rows, T.rowptr, T.col, T.val}};
    return 0;
  }
  std::vector<MuPiece> pieces;
  for (const CsrDev &S : T.segs) pieces.push_back(MuPiece{S.row0, S.rows, S.rowptr, S.col, S.val});
  HIP_TRY(hipMalloc((void **)&out.dev, sizeof(MuPiece) * pieces.size()));
  HIP_TRY(hipMemcpy(out.dev, pieces.data(), sizeof(MuPiece) * pieces.size(), hipMemcpyHostToDevice));
  out.src = MuSource{(int)pieces.size(), out.dev, pieces.front()};
  return 0;
}

// Every resident copy of one matrix takes its new values.  transpose != nullptr: D's CSR values come entry by entry from
// the transposed matrix (D = CSR(A) or CSR(Q)); nullptr: they are in place already (D = CSR(A') or CSR(Q'), the caller's
// order).  The derived copies then come from D's own CSR.
// EVERY COPY OF A MATRIX MUST APPEAR HERE AND IN apply_scaling's scale_one (abi_rescale.hpp): a layout added to one and
// not to the other keeps stale values after an update, or unscaled ones after a rescale.
static void place_matrix_values(pdhg_handle *h, CsrDev &D0, const MuSource *transpose) {
  std::function<void(CsrDev &)> place_one = [&](CsrDev &D) {
    for (CsrDev &S : D.segs) place_one(S);
    if (!D.segs.empty() || D.nnz == 0) return;
    if (transpose) {
      hipLaunchKernelGGL(mu_rows_kernel<true>, dim3(row_grid(D.rows)), dim3(TPB), 0, h->stream, D.rows, (const int *)D.rowptr,
                         (const int *)D.col, D.val, D.row0, *transpose, D.long_thr);
      if (D.nlong > 0)
        hipLaunchKernelGGL(mu_long_kernel<true>, dim3(D.nchunks), dim3(TPB), 0, h->stream, (const int *)D.rowptr, (const int *)D.col,
                           D.val, (const int *)D.chunk_row, (const int *)D.chunk_off, D.row0, *transpose);
    }
    const MuSource own{1, nullptr, MuPiece{0, D.rows, D.rowptr, D.col, D.val}};
    if (D.tiled && D.nwaves > 0)
      hipLaunchKernelGGL(mu_tiled_kernel<false>, dim3(row_grid(D.nwaves)), dim3(TPB), 0, h->stream, (const int2 *)D.wave_rows,
                         (const int *)D.wave_ent, (const int *)D.wave_step_off, (const int *)D.step_tile, (const int *)D.wg_step_off,
                         D.nwaves, D.tile_shift, (const unsigned *)D.pk, D.tv, 0, own);
    for (const SlabDev &S : D.slabs)
      if (S.nnz > 0)
        hipLaunchKernelGGL(mu_rows_kernel<false>, dim3(row_grid(D.rows)), dim3(TPB), 0, h->stream, D.rows, (const int *)S.rowptr,
                           (const int *)S.col, S.val, 0, own, 0);
    // the sliced jagged copies: copied again from the CSR arrays just refreshed (the same launch apply_scaling makes)
    auto refill = [&](const SjDev &J, const int *rowptr, const int *col, const double *val) {
      if (J.on() && J.nnz > 0)
        hipLaunchKernelGGL(sj_fill_kernel, dim3((J.nslices + TPB / WAVE - 1) / (TPB / WAVE)), dim3(TPB), 0, h->stream, J.nslices, (TPB / WAVE) * J.G,
                           (const unsigned *)J.meta, (const int *)J.slice_off, rowptr, col, val, J.col, J.val);
    };
    refill(D.sj, D.rowptr, D.col, D.val);
    for (const SlabDev &S : D.slabs) refill(S.sj, S.rowptr, S.col, S.val);
  };
  place_one(D0);
}

// the caller's values into CSR(A').val: one copy, or one per row segment (the segments cut the columns in order)
static int mu_upload_values(pdhg_handle *h, CsrDev &T, const double *vals) {
  int64_t off = 0;
  auto leaf = [&](CsrDev &S) -> int {
    if (S.nnz > 0) HIP_TRY(hipMemcpyAsync(S.val, vals + off, sizeof(double) * (size_t)S.nnz, hipMemcpyHostToDevice, h->stream));
    off += S.nnz;
    return 0;
  };
  if (T.segs.empty()) return leaf(T);
  for (CsrDev &S : T.segs) if (int rc = leaf(S)) return rc;
  return 0;
}

// Do the columns the handle was created from hold strictly ascending row indices?  (The searches need it.)  One read-only
// pass over the column indices of CSR(A') and CSR(Q'), made by a handle's first update and remembered.
static int mu_pattern_ascending(pdhg_handle *h) {
  if (h->csc_ascending >= 0) return 0;
  int *bad = nullptr, host_bad = 0;
  HIP_TRY(hipMalloc((void **)&bad, sizeof(int)));
  hipError_t e = hipMemsetAsync(bad, 0, sizeof(int), h->stream);
  std::function<void(const CsrDev &)> check = [&](const CsrDev &D) {
    for (const CsrDev &S : D.segs) check(S);
    if (!D.segs.empty() || D.nnz == 0) return;
    hipLaunchKernelGGL(mu_ascending_kernel<0>, dim3(row_grid(D.rows)), dim3(TPB), 0, h->stream, D.rows, (const int *)D.rowptr,
                       (const int *)D.col, bad);
  };
  if (e == hipSuccess) {
    check(h->At);
    if (h->has_q) check(h->Qt);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&host_bad, bad, sizeof(int), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(bad);
  if (e != hipSuccess) return fail_hip(e, "pdhg_update_matrix_values: checking the pattern");
  h->csc_ascending = host_bad ? 0 : 1;
  return 0;
}

int pdhg_update_matrix_values(pdhg_handle *h, int64_t nnz, const double *nzval, int64_t q_nnz, const double *q_nzval,
                              const double *c, const double *b, const double *lb, const double *ub) {
  RoctxRange roctx_range("pdhg_update_matrix_values");
  const std::string who = "pdhg_update_matrix_values";
  // every refusal first: nothing is launched, settled or written when one is reported
  int rc = resolve_refuse(h, who, true);
  if (rc) return rc;
  if (nnz != h->nnz)
    return fail(-1, who + ": nnz = " + std::to_string(nnz) + ", the handle was created with " + std::to_string(h->nnz) + " (the pattern is kept)");
  if (!nzval) return fail(-1, who + ": nzval == NULL");
  if (!c || !b || !lb || !ub) return fail(-1, who + ": c, b, lb and ub are all needed (the handle is not rescaled afterwards: they are the raw vectors)");
  if (!h->has_q && (q_nnz != 0 || q_nzval)) return fail(-1, who + ": q_nzval on a handle without an objective matrix (an update cannot turn an LP into a QP)");
  if (h->has_q && !q_nzval) return fail(-1, who + ": the handle has an objective matrix: q_nzval == NULL");
  if (h->has_q && q_nnz != h->Q.nnz)
    return fail(-1, who + ": q_nnz = " + std::to_string(q_nnz) + ", the objective matrix was set with " + std::to_string(h->Q.nnz));
  if ((rc = check_handle(h))) return rc;
  HIP_TRY(hipSetDevice(h->device));
  // (the one refusal that needs the device, and only on a handle's first update: a read-only pass)
  if ((rc = mu_pattern_ascending(h))) return rc;
  if (!h->csc_ascending)
    return fail(-1, who + ": the handle was created from columns whose row indices do not ascend strictly (unsorted or duplicate "
                          "entries): their values cannot be placed by search; create a new handle");
  const Shards L = shards_of(h);
  if ((rc = flush_pending(L))) return rc;

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
    // the raw vectors, as pdhg_create uploads them
    const struct { double *dst; const double *src; int64_t len; } vec[4] = {{h->c, c, h->n}, {h->b, b, h->m}, {h->lb, lb, h->n}, {h->ub, ub, h->n}};
    for (const auto &v : vec)
      if (v.len > 0) HIP_TRY(hipMemcpyAsync(v.dst, v.src, sizeof(double) * (size_t)v.len, hipMemcpyHostToDevice, h->stream));
    // the retained record starts again (its capacity stays: the pdhg_rescale that follows reuses it)
    ResolveState &R = *h->rs;
    R.steps = 0;
    hipLaunchKernelGGL(fill_kernel, dim3(h->ew_grid_n), dim3(TPB), 0, h->stream, (int)h->n, 1.0, R.cum_d);
    hipLaunchKernelGGL(fill_kernel, dim3(h->ew_grid_m), dim3(TPB), 0, h->stream, (int)h->m, 1.0, R.cum_e);
    HIP_TRY(hipGetLastError());
    return 0;
  };
  rc = body();
  // the evaluation caches and a fleet member's stored check results are keyed by these versions.  The point, the running
  // sums and the restart point are left as they are (flush_pending settled what was pending): they belong to the old
  // scaling, and the warm start every solve begins with empties them (resolve_clear_host is that call's).
  bump_version(L);
  h->matrix_version += 1;
  fleet_forget(h);
  // lb / ub are raw again, and a record of zero steps runs no apply_scaling that would rebuild their views
  const int rcb = bounds_rebuild(h);                    // (returns with the stream idle)
  if (rcb) (void)hipStreamSynchronize(h->stream);
  for (MuPiece *p : {from_at.dev, from_qt.dev}) if (p) (void)hipFree(p);
  return rc ? rc : rcb;
}
