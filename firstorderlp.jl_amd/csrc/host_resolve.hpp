// host_resolve.hpp -- part of the single translation unit pdhg_hip.hip (included there, after host_shards.hpp).
// RE-SOLVES on a live handle, host side: what the three forms of the C ABI stand on -- a handle of its own and a fleet
// (abi_resolve.hpp), a batch (abi_batch_resolve.hpp).  Each fact of the path is stated here once: what is retained, how
// the given vectors reach the device, which vectors a warm start zeroes, what a shared update leaves in a member, how a
// member takes its own A'y, what the last call did.  (ResolveCounters is declared beside pdhg_handle: FleetState holds it.)

// ---- what a retain hangs on a handle: a handle of its own, a fleet member, a batch (one for all its members) ----
struct ResolveState {
  int64_t steps = 0, cap = 0;                      // applied steps in the record / steps it has room for
  double *rec = nullptr;                           // [cap][n + m], device
  double *cum_d = nullptr, *cum_e = nullptr;       // the running products (n, m), 1.0 until a step is applied
  // one upload per call: the given vectors side by side in pinned memory, one copy to the device staging
  double *stage_host = nullptr, *stage_dev = nullptr;
};

// the retained record and the staging buffers of a handle (destroy_shard; the handle's device is current)
void resolve_release(pdhg_handle *h) {
  ResolveState *R = h->rs;
  if (!R) return;
  for (double *p : {R->rec, R->cum_d, R->cum_e, R->stage_dev}) if (p) (void)hipFree(p);
  if (R->stage_host) (void)hipHostFree(R->stage_host);
  delete R;
  h->rs = nullptr;
}

// pdhg_resolve_retain / pdhg_batch_resolve_retain behind their refusals: staging buffers of `stage_len` doubles
int resolve_retain(pdhg_handle *h, int64_t stage_len) {
  if (h->rs) return 0;
  int rc = check_handle(h, true, h->bat != nullptr);
  if (rc) return rc;
  const int64_t n = h->n, m = h->m;
  ResolveState *R = new ResolveState();
  h->rs = R;
  auto body = [&]() -> int {
    int r2;
    if ((r2 = alloc_zero(&R->cum_d, n))) return r2;
    if ((r2 = alloc_zero(&R->cum_e, m))) return r2;
    if ((r2 = alloc_zero(&R->stage_dev, stage_len))) return r2;
    HIP_TRY(hipHostMalloc((void **)&R->stage_host, sizeof(double) * (size_t)std::max<int64_t>(stage_len, 1), hipHostMallocDefault));
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

// ---- the given vectors side by side in a pinned buffer, uploaded in one copy: where the next one goes ----
struct ResolveStage {
  double *host;
  const double *dev;
  size_t off = 0;                                  // doubles placed so far
  // `len` doubles of `src` (nullptr: not given, nothing placed); returns where they will lie on the device, or nullptr
  const double *put(const double *src, int64_t len) {
    if (!src) return nullptr;
    if (len > 0) memcpy(host + off, src, sizeof(double) * (size_t)len);
    const double *at = dev + off;
    off += (size_t)len;
    return at;
  }
};

// one handle's part of a replay: its given vectors placed in the order c, lb, ub, b
ResolveReplayMember resolve_replay_member(pdhg_handle *h, ResolveStage &S, const double *c, const double *b, const double *lb, const double *ub) {
  ResolveReplayMember v{};
  v.in_c = S.put(c, h->n); v.in_lb = S.put(lb, h->n); v.in_ub = S.put(ub, h->n); v.in_b = S.put(b, h->m);
  v.c = h->c; v.lb = h->lb; v.ub = h->ub; v.b = h->b;
  return v;
}

// ---- a warm start ----
// The vectors a fresh handle holds zeros in: the running sums, their alternates, the restart point, a QP's kept Q x.
ResolveZeros resolve_fresh_zeros(const pdhg_handle *h) {
  ResolveZeros z{};
  z.zn[0] = h->sum_x; z.zn[1] = h->sum_x_alt; z.zn[2] = h->x_r; z.zn[3] = h->has_q ? h->qx : nullptr; z.zn[4] = h->has_q ? h->qx2 : nullptr;
  z.zm[0] = h->sum_y; z.zm[1] = h->sum_y_alt; z.zm[2] = h->y_r;
  return z;
}
// What it empties on the host side of one handle (the vectors are zeroed by the point kernel).
void resolve_clear_host(pdhg_handle *h) {
  drop_staging(h);
  h->pend_x = h->pend_y = false;             // a deferred update belongs to the sums being discarded
  h->pend_w = 0.0;
  h->sum_x_count = h->sum_y_count = 0;
  h->sum_x_weights = h->sum_y_weights = 0.0;
  h->restart_version += 1;                   // the restart point is zeros again: whatever was cached of the old one is stale
  h->state_version += 1;
  fleet_forget(h);
}
// this handle takes its own A'y of the y it was given
int resolve_own_aty(pdhg_handle *h) {
  const Shards L = shards_of(h);
  return dual_product(L, [](pdhg_handle *s) { return (const double *)s->y; }, [](pdhg_handle *s) { return s->aty; });
}

// ---- a member of a fleet or a batch after a shared update ----
// The evaluation caches and the stored check results are keyed by versions that do not see c / b / lb / ub.  K view
// rebuilds -- each a synchronisation, allocations and a round trip -- would undo the shared launch: the views are rebuilt
// where they are next read (bounds_fresh); the one-workgroup and the batched kernels read the dense arrays and never do.
void resolve_member_updated(pdhg_handle *h, bool bounds_touched) {
  h->state_version += 1;
  fleet_forget(h);
  if (bounds_touched) h->bnd_dirty = true;
}
// ... and such a rebuild, counted on the member's fleet
void resolve_count_view_rebuild(pdhg_handle *h) {
  if (h->fleet_of && h->fleet_of->fleet) h->fleet_of->fleet->rsv.other += 1;
}

// pdhg_fleet_resolve_info / pdhg_batch_resolve_info
void resolve_info(const ResolveCounters &c, int64_t out[4]) {
  out[0] = c.launches; out[1] = c.carried; out[2] = c.single; out[3] = c.other;
}
