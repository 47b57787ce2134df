// abi_resolve.hpp -- part of the single translation unit pdhg_hip.hip (included there, inside its extern "C" block, last).
// C ABI: RE-SOLVES on a live handle (include/pdhg_hip_resolve.h; kernels in resolve_kernels.hpp; what this form shares
// with a batch's, abi_batch_resolve.hpp, in host_resolve.hpp).  The matrix copies, the
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
  if (int rcw = batch_awaits_rescale(h, who + ": ")) return rcw;
  if (h->bat) return fail(-1, who + ": a batch handle is not supported by this call: a batch takes the pdhg_batch_ forms of pdhg_hip_batch_resolve.h");
  if (h->owner) return fail(-1, who + ": a batch member is not supported (it shares its batch's matrix and rescaling: call the pdhg_batch_ forms of pdhg_hip_batch_resolve.h on its batch)");
  if (h->grp) return fail(-1, who + ": a shard group is not supported");
  if (need_record && !h->rs) return fail(-1, who + ": pdhg_resolve_retain was not called on this handle before pdhg_rescale");
  return 0;
}

int pdhg_resolve_retain(pdhg_handle *h) {
  const int rc = resolve_refuse(h, "pdhg_resolve_retain", false);
  return rc ? rc : resolve_retain(h, 3 * h->n + h->m);
}

// the replay of one handle as kernel arguments, its given vectors placed at S
static ResolveReplayArgs resolve_replay_args(pdhg_handle *h, ResolveStage &S, const double *c, const double *b, const double *lb, const double *ub) {
  return ResolveReplayArgs{(int)h->n, (int)h->m, (int)h->rs->steps, h->rs->rec, resolve_replay_member(h, S, c, b, lb, ub)};
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
  ResolveStage S{R.stage_host, R.stage_dev};
  const ResolveReplayArgs a = resolve_replay_args(h, S, c, b, lb, ub);
  if (S.off > 0) HIP_TRY(hipMemcpyAsync(R.stage_dev, R.stage_host, sizeof(double) * S.off, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(resolve_replay_kernel, dim3(h->ew_grid_nm), dim3(TPB), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  // the evaluation caches and a fleet's stored check results are keyed by versions that do not see these four arrays
  bump_version(L);
  fleet_forget(h);
  if (lb || ub) return bounds_rebuild(h);             // (returns with the stream idle: the staging buffer is free again)
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

// the point kernel's arguments for one handle, its given vectors placed at S (x, then y)
static ResolvePointArgs resolve_point_args(pdhg_handle *h, ResolveStage &S, const double *x, const double *y) {
  const ResolveState &R = *h->rs;
  ResolvePointArgs a{};
  a.n = (int)h->n; a.m = (int)h->m; a.zero_aty = y ? 0 : 1;
  a.in_x = S.put(x, h->n); a.in_y = S.put(y, h->m);
  if (R.steps > 0) { a.cum_d = R.cum_d; a.cum_e = R.cum_e; }
  a.x = h->x; a.y = h->y; a.aty = h->aty;
  a.z = resolve_fresh_zeros(h);
  return a;
}

int pdhg_warm_start(pdhg_handle *h, const double *x, const double *y) {
  RoctxRange roctx_range("pdhg_warm_start");
  int rc = resolve_refuse(h, "pdhg_warm_start", true);
  if (rc) return rc;
  if ((rc = check_handle(h))) return rc;
  const Shards L = shards_of(h);
  ResolveState &R = *h->rs;
  ResolveStage S{R.stage_host, R.stage_dev};
  const ResolvePointArgs a = resolve_point_args(h, S, x, y);
  if (S.off > 0) HIP_TRY(hipMemcpyAsync(R.stage_dev, R.stage_host, sizeof(double) * S.off, hipMemcpyHostToDevice, h->stream));
  resolve_clear_host(h);
  hipLaunchKernelGGL(resolve_point_kernel, dim3(h->ew_grid_nm), dim3(TPB), 0, h->stream, a);
  HIP_TRY(hipGetLastError());
  if (y && (rc = resolve_own_aty(h))) return rc;
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
  F.rsv.carried = (int64_t)carried.size();
  F.rsv.single = 0;
  if (carried.empty()) return 0;
  HIP_TRY(hipSetDevice(fleet->device));
  const size_t item_bytes = sizeof(FleetResolveReplayItem) * n_items, bytes = item_bytes + sizeof(double) * n_data;
  if ((rc = fleet_resolve_reserve(fleet, bytes))) return rc;
  FleetResolveReplayItem *items = (FleetResolveReplayItem *)F.rsv_host;
  ResolveStage S{(double *)((char *)F.rsv_host + item_bytes), (const double *)((const char *)F.rsv_dev + item_bytes)};
  size_t placed = 0;
  for (int k : carried) {
    pdhg_handle *h = F.mem[(size_t)k];
    const double *pc = resolve_entry(c, k), *pb = resolve_entry(b, k), *pl = resolve_entry(lb, k), *pu = resolve_entry(ub, k);
    if ((rc = check_handle(h))) return rc;
    { Shards L = shards_of(h); if ((rc = flush_pending(L))) return rc; }
    const ResolveReplayArgs a = resolve_replay_args(h, S, pc, pb, pl, pu);
    const int64_t len = std::max(h->n, h->m);
    for (int64_t lo = 0; lo < len; lo += RESOLVE_CHUNK)
      items[placed++] = FleetResolveReplayItem{a, (int)lo, (int)std::min<int64_t>(lo + RESOLVE_CHUNK, len)};
  }
  if (placed > 0) {
    HIP_TRY(hipMemcpyAsync(F.rsv_dev, F.rsv_host, bytes, hipMemcpyHostToDevice, fleet->stream));
    hipLaunchKernelGGL(fleet_resolve_replay_kernel, dim3((unsigned)placed), dim3(TPB), 0, fleet->stream,
                       (const FleetResolveReplayItem *)F.rsv_dev, (int)placed);
    HIP_TRY(hipGetLastError());
    F.rsv.launches += 1;
  }
  for (int k : carried) resolve_member_updated(F.mem[(size_t)k], resolve_entry(lb, k) || resolve_entry(ub, k));
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
  F.rsv.carried = (int64_t)carried.size();
  F.rsv.single = 0;
  if (carried.empty()) return 0;
  HIP_TRY(hipSetDevice(fleet->device));
  const size_t item_bytes = sizeof(FleetResolvePointItem) * n_items, bytes = item_bytes + sizeof(double) * n_data;
  if ((rc = fleet_resolve_reserve(fleet, bytes))) return rc;
  FleetResolvePointItem *items = (FleetResolvePointItem *)F.rsv_host;
  ResolveStage S{(double *)((char *)F.rsv_host + item_bytes), (const double *)((const char *)F.rsv_dev + item_bytes)};
  size_t placed = 0;
  std::vector<FleetPointArgs> products;        // A'y of the members of the check class, in the launch pdhg_fleet_eval_points uses
  std::vector<int> own;                        // ... and the members that take their own (resolve_own_aty)
  for (int k : carried) {
    pdhg_handle *h = F.mem[(size_t)k];
    const double *px = resolve_entry(x, k), *py = resolve_entry(y, k);
    if ((rc = check_handle(h))) return rc;
    resolve_clear_host(h);
    const ResolvePointArgs a = resolve_point_args(h, S, px, py);
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
    F.rsv.launches += 1;
  }
  if ((rc = fleet_check_launch(fleet, 0, products, fleet_point_products_kernel, TPB, 0))) return rc;
  F.rsv.single = (int64_t)own.size();
  for (int k : own)
    if ((rc = resolve_own_aty(F.mem[(size_t)k]))) return rc;
  HIP_TRY(hipStreamSynchronize(fleet->stream));
  return 0;
}

int pdhg_fleet_resolve_info(pdhg_handle *fleet, int64_t out[4]) {
  if (!out) return fail(-1, "out == NULL");
  if (!fleet_of(fleet)) return fail(-1, "pdhg_fleet_resolve_info: not a fleet handle");
  resolve_info(fleet->fleet->rsv, out);
  return 0;
}
