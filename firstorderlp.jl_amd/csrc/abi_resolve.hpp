// abi_resolve.hpp -- part of the single translation unit pdhg_hip.hip (included there, inside its extern "C" block, last).
// C ABI: RE-SOLVES on a live handle (include/pdhg_hip_resolve.h; kernels in resolve_kernels.hpp).  The matrix copies, the
// layouts and the rescaling factors depend on A and Q only: a caller who solves the same matrix again with other vectors
// keeps the handle, sends the new c / b / lb / ub in the space pdhg_create took them in, and names a starting point.
//
//   pdhg_resolve_retain            before pdhg_rescale: every apply_scaling step appends its factors to a record
//   pdhg_update_problem_vectors    one upload, one launch that replays the recorded steps on the new vectors
//   pdhg_warm_start                one upload, one launch: the point to the working space, everything a fresh handle has
//                                  empty emptied; then A'y
//   pdhg_fleet_*                   the same for the members of a fleet, each call ONE shared launch over (member, chunk) items
//
// State a warm start clears: the running sums, their counts and weights; the alternates of the paired
// average update and its staging; a pending lazy accept; the saved restart point (restart_version moves on); a QP's
// kept Q x (both buffers); the versions that key the evaluation caches; a fleet member's stored check results.  The step
// kernels carry nothing else from launch to launch: their control words are keyed by epochs and sequence numbers that
// only ever advance, and the trial buffers are written before they are read.

static int resolve_refuse(pdhg_handle *h, const std::string &who, bool need_record) {
  if (!h) return fail(-1, who + ": null handle");
  if (h->fleet) return fail(-1, who + ": a fleet handle holds no problem of its own: call the pdhg_fleet_ form, or this on a member");
  if (h->bat) return fail(-1, who + ": a batch handle is not supported by this call: a batch takes the pdhg_batch_ forms of pdhg_hip_batch_resolve.h");
  if (h->owner) return fail(-1, who + ": a batch member is not supported (it shares its batch's matrix and rescaling: call the pdhg_batch_ forms of pdhg_hip_batch_resolve.h on its batch)");
  if (h->grp) return fail(-1, who + ": a shard group is not supported");
  if (need_record && !h->rs) return fail(-1, who + ": pdhg_resolve_retain was not called on this handle before pdhg_rescale");
  return 0;
}

int pdhg_resolve_retain(pdhg_handle *h) {
  int rc = resolve_refuse(h, "pdhg_resolve_retain", false);
  if (rc) return rc;
  if (h->rs) return 0;
  if ((rc = check_handle(h))) return rc;
  const int64_t n = h->n, m = h->m;
  ResolveState *R = new ResolveState();
  h->rs = R;
  auto body = [&]() -> int {
    int r2;
    if ((r2 = alloc_zero(&R->cum_d, n))) return r2;
    if ((r2 = alloc_zero(&R->cum_e, m))) return r2;
    if ((r2 = alloc_zero(&R->stage_dev, 3 * n + m))) return r2;
    HIP_TRY(hipHostMalloc((void **)&R->stage_host, sizeof(double) * (size_t)std::max<int64_t>(3 * n + m, 1), hipHostMallocDefault));
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

// the replay of one handle as kernel arguments: `in` = where the given vectors lie on the device, in the order c, lb, ub, b
// (only the given ones, side by side)
static ResolveReplayArgs resolve_replay_args(pdhg_handle *h, const double *in, bool gc, bool gb, bool gl, bool gu) {
  const ResolveState &R = *h->rs;
  ResolveReplayArgs a{};
  a.n = (int)h->n; a.m = (int)h->m; a.steps = (int)R.steps; a.rec = R.rec;
  if (gc) { a.in_c = in; in += h->n; }
  if (gl) { a.in_lb = in; in += h->n; }
  if (gu) { a.in_ub = in; in += h->n; }
  if (gb) { a.in_b = in; in += h->m; }
  a.c = h->c; a.lb = h->lb; a.ub = h->ub; a.b = h->b;
  return a;
}
// ... and the same vectors packed into `dst` (host); returns the doubles written
static int64_t resolve_pack_vectors(const pdhg_handle *h, double *dst, const double *c, const double *b, const double *lb, const double *ub) {
  int64_t off = 0;
  auto put = [&](const double *src, int64_t len) {
    if (!src) return;
    if (len > 0) memcpy(dst + off, src, sizeof(double) * (size_t)len);
    off += len;
  };
  put(c, h->n); put(lb, h->n); put(ub, h->n); put(b, h->m);
  return off;
}

int pdhg_update_problem_vectors(pdhg_handle *h, const double *c, const double *b, const double *lb, const double *ub) {
  RoctxRange roctx_range("pdhg_update_problem_vectors");
  int rc = resolve_refuse(h, "pdhg_update_problem_vectors", true);
  if (rc) return rc;
  if (!c && !b && !lb && !ub) return 0;
  if ((rc = check_handle(h))) return rc;
  const Shards L = shards_of(h);
  if ((rc = flush_pending(L))) return rc;
  ResolveState &R = *h->rs;
  const int64_t len = resolve_pack_vectors(h, R.stage_host, c, b, lb, ub);
  if (len > 0) HIP_TRY(hipMemcpyAsync(R.stage_dev, R.stage_host, sizeof(double) * (size_t)len, hipMemcpyHostToDevice, h->stream));
  const ResolveReplayArgs a = resolve_replay_args(h, R.stage_dev, c != nullptr, b != nullptr, lb != nullptr, ub != nullptr);
  hipLaunchKernelGGL(resolve_replay_kernel, dim3(h->ew_grid_nm), dim3(TPB), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  // the evaluation caches and a fleet's stored check results are keyed by versions that do not see these four arrays
  bump_version(L);
  fleet_forget(h);
  if (lb || ub) return bounds_rebuild(h);             // (returns with the stream idle: the staging buffer is free again)
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

// What a warm start empties on the host side of one handle (the vectors are zeroed by the point kernel).
static void resolve_clear_host(pdhg_handle *h) {
  drop_staging(h);
  h->pend_x = h->pend_y = false;             // a deferred update belongs to the sums being discarded
  h->pend_w = 0.0;
  h->sum_x_count = h->sum_y_count = 0;
  h->sum_x_weights = h->sum_y_weights = 0.0;
  h->restart_version += 1;                   // the restart point is zeros again: whatever was cached of the old one is stale
  h->state_version += 1;
  fleet_forget(h);
}
// the point kernel's arguments for one handle: `in` = the given vectors on the device, x then y (only the given ones)
static ResolvePointArgs resolve_point_args(pdhg_handle *h, const double *in, bool gx, bool gy) {
  const ResolveState &R = *h->rs;
  ResolvePointArgs a{};
  a.n = (int)h->n; a.m = (int)h->m; a.zero_aty = gy ? 0 : 1;
  if (gx) { a.in_x = in; in += h->n; }
  if (gy) { a.in_y = in; in += h->m; }
  if (R.steps > 0) { a.cum_d = R.cum_d; a.cum_e = R.cum_e; }
  a.x = h->x; a.y = h->y; a.aty = h->aty;
  a.zn[0] = h->sum_x; a.zn[1] = h->sum_x_alt; a.zn[2] = h->x_r; a.zn[3] = h->has_q ? h->qx : nullptr; a.zn[4] = h->has_q ? h->qx2 : nullptr;
  a.zm[0] = h->sum_y; a.zm[1] = h->sum_y_alt; a.zm[2] = h->y_r;
  return a;
}

int pdhg_warm_start(pdhg_handle *h, const double *x, const double *y) {
  RoctxRange roctx_range("pdhg_warm_start");
  int rc = resolve_refuse(h, "pdhg_warm_start", true);
  if (rc) return rc;
  if ((rc = check_handle(h))) return rc;
  const Shards L = shards_of(h);
  ResolveState &R = *h->rs;
  int64_t len = 0;
  if (x) { if (h->n > 0) memcpy(R.stage_host, x, sizeof(double) * (size_t)h->n); len += h->n; }
  if (y) { if (h->m > 0) memcpy(R.stage_host + len, y, sizeof(double) * (size_t)h->m); len += h->m; }
  if (len > 0) HIP_TRY(hipMemcpyAsync(R.stage_dev, R.stage_host, sizeof(double) * (size_t)len, hipMemcpyHostToDevice, h->stream));
  resolve_clear_host(h);
  const ResolvePointArgs a = resolve_point_args(h, R.stage_dev, x != nullptr, y != nullptr);
  hipLaunchKernelGGL(resolve_point_kernel, dim3(h->ew_grid_nm), dim3(TPB), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  if (y && (rc = dual_product(L, [](pdhg_handle *s) { return (const double *)s->y; }, [](pdhg_handle *s) { return s->aty; }))) return rc;
  return sync_all(L);
}

// ---- the fleet forms -------------------------------------------------------------------------------------------------
// One table per call in pinned memory -- the (member, chunk) items, then the members' vectors -- uploaded once, one launch.

static int fleet_resolve_reserve(pdhg_handle *f, size_t bytes) {
  FleetState &F = *f->fleet;
  if (F.rsv_cap >= bytes) return 0;
  HIP_TRY(hipStreamSynchronize(f->stream));
  if (F.rsv_dev) (void)hipFree(F.rsv_dev);
  if (F.rsv_host) (void)hipHostFree(F.rsv_host);
  F.rsv_dev = F.rsv_host = nullptr;
  F.rsv_cap = 0;
  const size_t cap = std::max<size_t>(2 * bytes, 4096);
  HIP_TRY(hipMalloc(&F.rsv_dev, cap));
  HIP_TRY(hipHostMalloc(&F.rsv_host, cap, hipHostMallocDefault));
  F.rsv_cap = cap;
  return 0;
}
static int64_t resolve_chunks(const pdhg_handle *h) {
  return (std::max(h->n, h->m) + RESOLVE_CHUNK - 1) / RESOLVE_CHUNK;
}
static const double *resolve_entry(const double *const *arr, int k) { return arr ? arr[k] : nullptr; }

int pdhg_fleet_update_problem_vectors(pdhg_handle *fleet, const double *const *c, const double *const *b,
                                      const double *const *lb, const double *const *ub) {
  RoctxRange roctx_range("pdhg_fleet_update_problem_vectors");
  if (!fleet) return fail(-1, "null handle");
  if (!fleet_of(fleet)) return fail(-1, "pdhg_fleet_update_problem_vectors: not a fleet handle");
  FleetState &F = *fleet->fleet;
  const int K = (int)F.mem.size();
  int rc;
  // every refusal first: nothing has been touched when one is reported
  std::vector<int> carried;
  size_t n_items = 0, n_data = 0;
  for (int k = 0; k < K; ++k) {
    const double *pc = resolve_entry(c, k), *pb = resolve_entry(b, k), *pl = resolve_entry(lb, k), *pu = resolve_entry(ub, k);
    if (!pc && !pb && !pl && !pu) continue;
    pdhg_handle *h = F.mem[(size_t)k];
    if ((rc = resolve_refuse(h, "pdhg_fleet_update_problem_vectors: member " + std::to_string(k), true))) return rc;
    carried.push_back(k);
    n_items += (size_t)resolve_chunks(h);
    n_data += (size_t)((pc ? h->n : 0) + (pl ? h->n : 0) + (pu ? h->n : 0) + (pb ? h->m : 0));
  }
  F.rsv_carried = (int64_t)carried.size();
  F.rsv_single = 0;
  if (carried.empty()) return 0;
  HIP_TRY(hipSetDevice(fleet->device));
  const size_t item_bytes = sizeof(FleetResolveReplayItem) * n_items, bytes = item_bytes + sizeof(double) * n_data;
  if ((rc = fleet_resolve_reserve(fleet, bytes))) return rc;
  FleetResolveReplayItem *items = (FleetResolveReplayItem *)F.rsv_host;
  double *data_host = (double *)((char *)F.rsv_host + item_bytes);
  const double *data_dev = (const double *)((const char *)F.rsv_dev + item_bytes);
  size_t placed = 0, off = 0;
  for (int k : carried) {
    pdhg_handle *h = F.mem[(size_t)k];
    const double *pc = resolve_entry(c, k), *pb = resolve_entry(b, k), *pl = resolve_entry(lb, k), *pu = resolve_entry(ub, k);
    if ((rc = check_handle(h))) return rc;
    { Shards L = shards_of(h); if ((rc = flush_pending(L))) return rc; }
    const ResolveReplayArgs a = resolve_replay_args(h, data_dev + off, pc != nullptr, pb != nullptr, pl != nullptr, pu != nullptr);
    off += (size_t)resolve_pack_vectors(h, data_host + off, pc, pb, pl, pu);
    const int64_t len = std::max(h->n, h->m);
    for (int64_t lo = 0; lo < len; lo += RESOLVE_CHUNK)
      items[placed++] = FleetResolveReplayItem{a, (int)lo, (int)std::min<int64_t>(lo + RESOLVE_CHUNK, len)};
  }
  if (placed > 0) {
    HIP_TRY(hipMemcpyAsync(F.rsv_dev, F.rsv_host, bytes, hipMemcpyHostToDevice, fleet->stream));
    hipLaunchKernelGGL(fleet_resolve_replay_kernel, dim3((unsigned)placed), dim3(TPB), 0, fleet->stream,
                       (const FleetResolveReplayItem *)F.rsv_dev, (int)placed);
    HIP_TRY(hipGetLastError());
    F.rsv_launches += 1;
  }
  for (int k : carried) {
    pdhg_handle *h = F.mem[(size_t)k];
    h->state_version += 1;
    fleet_forget(h);
    // K view rebuilds -- each a synchronisation, allocations and a round trip -- would undo the shared launch: the views
    // are rebuilt where they are next read (bounds_fresh); the one-workgroup kernels read the dense arrays and never do
    if (resolve_entry(lb, k) || resolve_entry(ub, k)) h->bnd_dirty = true;
  }
  HIP_TRY(hipStreamSynchronize(fleet->stream));         // (the table is free for the next call)
  return 0;
}

int pdhg_fleet_warm_start(pdhg_handle *fleet, const double *const *x, const double *const *y) {
  RoctxRange roctx_range("pdhg_fleet_warm_start");
  if (!fleet) return fail(-1, "null handle");
  if (!fleet_of(fleet)) return fail(-1, "pdhg_fleet_warm_start: not a fleet handle");
  FleetState &F = *fleet->fleet;
  const int K = (int)F.mem.size();
  const bool everyone = !x && !y;               // NULL arrays: zeros for every member; a member with two NULL entries is left alone
  int rc;
  std::vector<int> carried;
  size_t n_items = 0, n_data = 0;
  for (int k = 0; k < K; ++k) {
    const double *px = resolve_entry(x, k), *py = resolve_entry(y, k);
    if (!everyone && !px && !py) continue;
    pdhg_handle *h = F.mem[(size_t)k];
    if ((rc = resolve_refuse(h, "pdhg_fleet_warm_start: member " + std::to_string(k), true))) return rc;
    carried.push_back(k);
    n_items += (size_t)resolve_chunks(h);
    n_data += (size_t)((px ? h->n : 0) + (py ? h->m : 0));
  }
  F.rsv_carried = (int64_t)carried.size();
  F.rsv_single = 0;
  if (carried.empty()) return 0;
  HIP_TRY(hipSetDevice(fleet->device));
  const size_t item_bytes = sizeof(FleetResolvePointItem) * n_items, bytes = item_bytes + sizeof(double) * n_data;
  if ((rc = fleet_resolve_reserve(fleet, bytes))) return rc;
  FleetResolvePointItem *items = (FleetResolvePointItem *)F.rsv_host;
  double *data_host = (double *)((char *)F.rsv_host + item_bytes);
  const double *data_dev = (const double *)((const char *)F.rsv_dev + item_bytes);
  size_t placed = 0, off = 0;
  std::vector<FleetPointArgs> products;        // A'y of the members of the check class, in the launch pdhg_fleet_eval_points uses
  std::vector<int> own;                        // ... and the members served by their own dual_product
  for (int k : carried) {
    pdhg_handle *h = F.mem[(size_t)k];
    const double *px = resolve_entry(x, k), *py = resolve_entry(y, k);
    if ((rc = check_handle(h))) return rc;
    resolve_clear_host(h);
    const ResolvePointArgs a = resolve_point_args(h, data_dev + off, px != nullptr, py != nullptr);
    if (px) { if (h->n > 0) memcpy(data_host + off, px, sizeof(double) * (size_t)h->n); off += (size_t)h->n; }
    if (py) { if (h->m > 0) memcpy(data_host + off, py, sizeof(double) * (size_t)h->m); off += (size_t)h->m; }
    const int64_t len = std::max(h->n, h->m);
    for (int64_t lo = 0; lo < len; lo += RESOLVE_CHUNK)
      items[placed++] = FleetResolvePointItem{a, (int)lo, (int)std::min<int64_t>(lo + RESOLVE_CHUNK, len)};
    if (!py) continue;
    if (fleet_check_eligible(h)) {
      // fleet_point_products_kernel's rows are bit for bit launch_spmv<MODE_PLAIN>'s for this class: A'y straight into
      // the iterate's product, A x (which the kernel also computes) into scratch
      FleetPointArgs p{};
      p.n = (int)h->n; p.m = (int)h->m; p.do_products = 1;
      p.A = h->A.view(); p.T = h->At.view();
      p.px = h->x; p.py = h->y; p.ax = h->tmp_m; p.aty = h->aty;
      products.push_back(p);
    } else own.push_back(k);
  }
  if (placed > 0) {
    HIP_TRY(hipMemcpyAsync(F.rsv_dev, F.rsv_host, bytes, hipMemcpyHostToDevice, fleet->stream));
    hipLaunchKernelGGL(fleet_resolve_point_kernel, dim3((unsigned)placed), dim3(TPB), 0, fleet->stream,
                       (const FleetResolvePointItem *)F.rsv_dev, (int)placed);
    HIP_TRY(hipGetLastError());
    F.rsv_launches += 1;
  }
  if ((rc = fleet_check_launch(fleet, 0, products, fleet_point_products_kernel, TPB, 0))) return rc;
  F.rsv_single = (int64_t)own.size();
  for (int k : own) {
    pdhg_handle *h = F.mem[(size_t)k];
    Shards L = shards_of(h);
    if ((rc = dual_product(L, [](pdhg_handle *s) { return (const double *)s->y; }, [](pdhg_handle *s) { return s->aty; }))) return rc;
  }
  HIP_TRY(hipStreamSynchronize(fleet->stream));
  return 0;
}

int pdhg_fleet_resolve_info(pdhg_handle *fleet, int64_t out[4]) {
  if (!out) return fail(-1, "out == NULL");
  if (!fleet_of(fleet)) return fail(-1, "pdhg_fleet_resolve_info: not a fleet handle");
  const FleetState &F = *fleet->fleet;
  out[0] = F.rsv_launches; out[1] = F.rsv_carried; out[2] = F.rsv_single; out[3] = F.rsv_view_rebuilds;
  return 0;
}
