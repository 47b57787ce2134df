// host_checks.hpp -- part of the single translation unit pdhg_hip.hip (included there, after host_resolve.hpp).
// A CHECK is a termination evaluation or a trust-region bound at the CURRENT, AVERAGE or RESTART point.  It has three host
// paths -- one handle (abi_eval.hpp), a fleet's shared launches (abi_fleet_checks.hpp), a batch's (abi_batch_checks.hpp) --
// that must agree on bits and on cache keys.  What they share is stated here, once: which buffers a point names and
// what is stale there (claim_point), the refusals, the 28 result words, the argument blocks of the shared kernels, and
// the small host chores around them.  The paths differ in who does the work a claim asks for, not in what is asked.

// ---- buffers and result words ------------------------------------------------------------------------------------------

static int ev_alloc(pdhg_handle *h) {
  if (h->ev_partials) return 0;
  int rc;
  {
    // the evaluation kernels reduce up to 30 quantities per workgroup and a second stage reads every workgroup's
    // partials: two elements per thread and at most 1024 workgroups measured best (L1-SVM 229K elements: 448
    // workgroups 67 us per trust-region call against 82 with 895; 2M elements: 977 workgroups 123 us against 147 with 2048)
    static const int per_thread = dev_env("PDHG_EV_ELEMS") ? std::max(1, atoi(dev_env("PDHG_EV_ELEMS"))) : 2;
    h->ev_grid = std::min(1024, ew_grid((h->n + h->m + per_thread) / per_thread));
  }
  if ((rc = alloc_zero(&h->ev_partials, (int64_t)EV_MAXQ * h->ev_grid))) return rc;
  if ((rc = alloc_zero(&h->ev_ax, h->m))) return rc;
  if ((rc = alloc_zero(&h->ev_aty, h->n_alloc))) return rc;
  for (int k = 0; k < 3; ++k) {
    if ((rc = alloc_zero(&h->ev_cax[k], h->m))) return rc;
    if ((rc = alloc_zero(&h->ev_caty[k], h->n_alloc))) return rc;
  }
  if (h->grp && (rc = alloc_zero(&h->ev_xg, h->n_alloc))) return rc;
  if ((rc = alloc_zero(&h->px_avg, h->n))) return rc;
  if ((rc = alloc_zero(&h->py_avg, h->m))) return rc;
  if ((rc = alloc_zero(&h->x_r, h->n))) return rc;   // zeros == the initial restart point (pdhg.jl:869)
  if ((rc = alloc_zero(&h->y_r, h->m))) return rc;
  return 0;
}

// Pinned result words a kernel publishes into and the host polls (grid_sync.hpp: publish_words / wait_words): per item
// EV_HOST_SLOTS values, checksum, sequence number, zeroed.  At least `items` of them; a block that has to grow is freed
// once `stream` has drained (a launch may still publish into it).
static int ensure_result_words(double **res, size_t *cap, size_t items, hipStream_t stream) {
  if (*cap >= items) return 0;
  if (*res) {
    HIP_TRY(hipStreamSynchronize(stream));
    (void)hipHostFree(*res);
    *res = nullptr;
    *cap = 0;
  }
  const size_t bytes = items * (EV_HOST_SLOTS + 2) * sizeof(double);
  HIP_TRY(hipHostMalloc((void **)res, bytes, hipHostMallocCoherent | hipHostMallocMapped));
  memset(*res, 0, bytes);
  *cap = items;
  return 0;
}
// one handle's own (multi_final_kernel, tr_small_kernel, the shared evaluation kernels)
static int ev_ensure_host(pdhg_handle *h) {
  size_t cap = h->ev_host ? 1 : 0;
  return ensure_result_words(&h->ev_host, &cap, 1, h->stream);
}
static int ev_wait_host(pdhg_handle *h, int k, unsigned long long seq, double *out) {
  return wait_words(h->stream, h->ev_host, EV_HOST_SLOTS, k, seq, out, 40000000L,
                    "evaluation reduction finished without publishing its results");
}

// ---- which form of the evaluation is in force --------------------------------------------------------------------------

// The evaluation reductions publish into pinned host memory (one handle) unless PDHG_EVAL_HOST_WORD=0 (dev): decided in
// ONE place and per call -- pdhg_eval_point's combined 22-quantity reduction (which needs the max mask) and ev_finish
// must never disagree (a cached copy here once could: sums where maxima belong).
static bool eval_host_word() {
  const char *hw = dev_env("PDHG_EVAL_HOST_WORD");
  return !(hw && hw[0] == '0');
}
// the distances of a check ride in the evaluation's reduction (dev knob, read per call: tests compare both forms in one process)
static bool eval_prefetch() {
  const char *pf = dev_env("PDHG_EVAL_PREFETCH");
  return !(pf && pf[0] == '0');
}
// The shared evaluation kernels restate the one-handle form with its prefetched distances and the per-point caches: with
// one of its development switches set a fleet or a batch serves every member by the member's own call.
static bool eval_shared_form_in_force() {
  return eval_host_word() && eval_prefetch() && dev_env("PDHG_NO_EVAL_CACHE") == nullptr;
}

// ---- a point and what is stale at it -----------------------------------------------------------------------------------

// slot of the per-point buffers: 0 CURRENT, 1 AVERAGE, 2 RESTART (anything else: point_error refuses it first)
static int point_index(int point) {
  if (point == PDHG_POINT_CURRENT) return 0;
  return point == PDHG_POINT_AVERAGE ? 1 : 2;
}

// the refusals of a point selector, `who` (if any) in front
static int point_error(const pdhg_handle *h, int point, const std::string &who) {
  const std::string pre = who.empty() ? who : who + ": ";
  if (point != PDHG_POINT_CURRENT && point != PDHG_POINT_AVERAGE && point != PDHG_POINT_RESTART)
    return fail(-1, pre + "unknown point selector");
  if (point == PDHG_POINT_AVERAGE && (h->sum_x_count == 0 || h->sum_y_count == 0)) return fail(-1, pre + "average is empty");
  return 0;
}

// The freshness marks of the handles a shared call claims points of, as they were before.  claim_point marks a cache fresh
// at once -- a later item of the same call at the same point of the same member must find it so -- but nothing has filled
// it until the call's product launches have been issued: a call that returns with an error before that (a later member's
// flush_pending, a table that cannot be allocated, the launch itself) puts the marks back, and the member's next call
// computes.  (ev_seq only ever advances: a number no kernel published is never waited for again.)
struct CheckMarks {
  struct Saved { pdhg_handle *h; uint64_t avg_version, cversion[2], rkey; };
  std::vector<Saved> saved;
  bool issued = false;
  void keep(pdhg_handle *h) {
    for (const Saved &s : saved) if (s.h == h) return;
    saved.push_back(Saved{h, h->avg_version, {h->ev_cversion[0], h->ev_cversion[1]}, h->ev_rkey});
  }
  ~CheckMarks() {
    if (issued) return;
    for (const Saved &s : saved) {
      s.h->avg_version = s.avg_version; s.h->ev_cversion[0] = s.cversion[0]; s.h->ev_cversion[1] = s.cversion[1]; s.h->ev_rkey = s.rkey;
    }
  }
};

// a point's vectors (px: column vector, valid on the owned slice; py: this shard's rows) and where its products live
struct PointRef { const double *px, *py; double *ax, *aty, *qx; };
// ... and the work the claim leaves to its caller: materialise the average first / compute the products
struct PointClaim : PointRef { bool need_div, stale; };
// the point point_products left in the handle
static PointRef point_in_handle(const pdhg_handle *h) { return PointRef{h->pt_x, h->pt_y, h->pt_ax, h->pt_aty, h->pt_qx}; }

// Bookkeeping of `point` on one handle, without a launch: its buffers, whether the average has to be materialised
// (avg_version), and -- products == true -- whether A x, A' y (Q x) in the per-point buffers are stale: CURRENT and AVERAGE
// hold for one state_version, RESTART until the restart point or the matrix changes, and Q x is allocated on first use,
// which makes the products stale.  All of it is marked fresh here; the caller issues what the claim asks for (and hands
// `marks` when it can fail before it has).  products == false: the average only, for the evaluation's distances.
// products == true also leaves the point in h->pt_*; every reader of pt_* claims its point itself first (point_products,
// select_point), so a fleet's or a batch's claim on a member is never read from there by mistake.
static int claim_point(pdhg_handle *h, int point, bool products, CheckMarks *marks, PointClaim *c) {
  int rc;
  if ((rc = ev_alloc(h))) return rc;
  if ((rc = point_error(h, point, ""))) return rc;
  if (marks) marks->keep(h);
  const int k = point_index(point);
  const double *const xs[3] = {h->x, h->px_avg, h->x_r}, *const ys[3] = {h->y, h->py_avg, h->y_r};
  c->px = xs[k]; c->py = ys[k]; c->ax = h->ev_cax[k]; c->aty = h->ev_caty[k];
  c->need_div = k == 1 && h->avg_version != h->state_version;
  if (c->need_div) h->avg_version = h->state_version;
  c->stale = false;
  if (products) {
    if (k < 2) {
      c->stale = h->ev_cversion[k] != h->state_version;
      h->ev_cversion[k] = h->state_version;
    } else {
      const uint64_t key = (h->matrix_version << 32) + h->restart_version;
      c->stale = h->ev_rkey != key;
      h->ev_rkey = key;
    }
    if (h->has_q && !h->ev_cqx[k]) {
      if ((rc = alloc_zero(&h->ev_cqx[k], h->n))) return rc;
      c->stale = true;
    }
  }
  c->qx = h->has_q ? h->ev_cqx[k] : nullptr;
  if (products) { h->pt_x = c->px; h->pt_y = c->py; h->pt_ax = c->ax; h->pt_aty = c->aty; h->pt_qx = c->qx; }
  return 0;
}

// ---- the evaluation's 28 result words ----------------------------------------------------------------------------------

// quantities 0-3 sums, 4-7 maxes (rows); 8-14 sums, 15-21 maxes (columns) -> out[24]; 22-27 (prefetched == true) the
// scalars the rest of the check asks for next, kept in the handle for pdhg_distance_to_restart / pdhg_point_sumsq
static void eval_unpack(pdhg_handle *h, int point, bool prefetched, bool have_avg, const double *r, double out[24]) {
  if (prefetched) {
    for (int q = 0; q < 6; ++q) h->chk_vals[q] = r[22 + q];
    h->chk_state = h->state_version;
    h->chk_restart = h->restart_version;
    h->chk_point = point;
    h->chk_have_avg = have_avg;
  }
  for (int q = 0; q < 8; ++q) out[q] = r[q];
  for (int q = 0; q < 6; ++q) { out[8 + q] = r[8 + q]; out[14 + q] = r[8 + 7 + q]; }
  out[20] = r[8 + 6]; out[21] = r[8 + 13]; out[22] = out[23] = 0.0;
}

// ---- argument blocks of the shared kernels -----------------------------------------------------------------------------

// one member's evaluation at the claimed point `pt` (fleet_qp_eval_kernel, the batch's evaluation kernels; an LP member
// of a fleet takes the FleetEvalArgs part)
static FleetQpEvalArgs eval_args_of(const pdhg_handle *h, const PointRef &pt, bool have_avg, double *host_out, unsigned long long seq) {
  FleetQpEvalArgs a{};
  a.n = (int)h->n; a.m = (int)h->m; a.ne = (int)h->num_eq; a.grid = h->ev_grid; a.have_avg = have_avg ? 1 : 0;
  a.pt_x = pt.px; a.pt_y = pt.py; a.pt_ax = pt.ax; a.pt_aty = pt.aty; a.pt_qx = pt.qx;
  a.E = h->E; a.b_o = h->b_o; a.Dv = h->Dv; a.c_o = h->c_o; a.lb_o = h->lb_o; a.ub_o = h->ub_o;
  a.avg_x = have_avg ? h->px_avg : nullptr; a.avg_y = have_avg ? h->py_avg : nullptr;
  a.x = h->x; a.y = h->y; a.x_r = h->x_r; a.y_r = h->y_r;
  a.partials = h->ev_partials; a.scal = h->scal_dev;
  a.host_out = host_out;
  a.seq = seq;
  return a;
}

// the trust-region problem at `pt` into the fields TrSmallArgs and TrCoopArgs share
template <class Args>
static void tr_problem_fill(Args &a, const pdhg_handle *h, const PointRef &pt, double wp, double wd, double radius, int range,
                            int approximate) {
  a.n = (int)h->n; a.m = (int)h->m; a.ne = (int)h->num_eq; a.range = range; a.approximate = approximate ? 1 : 0;
  a.px = pt.px; a.py = pt.py; a.aty = pt.aty; a.qx = pt.qx; a.ax = pt.ax;
  a.c = h->c; a.b = h->b; a.lb = h->lb; a.ub = h->ub;
  a.wp = wp; a.wd = wd; a.radius = radius;
}

// A kernel's dynamic-LDS limit, raised per device to the largest request so far (one instance per kernel).
struct DynLdsLimit {
  const void *kernel;
  size_t limit[64] = {};
  std::mutex mu;
  int raise(int device, size_t lds) {
    std::lock_guard<std::mutex> lock(mu);
    size_t &cur = limit[device & 63];
    if (cur < lds) {
      HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      cur = lds;
    }
    return 0;
  }
};
static DynLdsLimit tr_small_lds{(const void *)tr_small_kernel}, fleet_tr_lds{(const void *)fleet_tr_kernel};
static DynLdsLimit fleet_rescale_lds{(const void *)fleet_rescale_kernel};      // (abi_fleet_rescale.hpp)

// ---- a member a shared call does not carry -----------------------------------------------------------------------------

// Served by its own call inside the shared one: the stored result is invalidated first (the member's call computes: never
// an answer from an earlier shared call), `serving` is up meanwhile (no miss of the caller's), and the result is stored
// with the member as a carried one is.
static int serve_eval_by_own_call(bool &serving, pdhg_handle *h, int point, double *out) {
  h->fc_eval.valid = false;
  serving = true;
  const int rc = pdhg_eval_point(h, point, out);
  serving = false;
  if (rc) return rc;
  fleet_store_eval(h, point, out);
  return 0;
}
static int serve_tr_by_own_call(bool &serving, pdhg_handle *h, int point, double wp, double wd, double radius, int range,
                                int approximate, double *out) {
  for (pdhg_handle::FleetTrResult &r : h->fc_tr)
    if (fleet_tr_same(h, r, point, wp, wd, radius, range, approximate)) r.valid = false;
  serving = true;
  const int rc = pdhg_trust_region_bound(h, point, wp, wd, radius, range, approximate, out);
  serving = false;
  if (rc) return rc;
  fleet_store_tr(h, point, wp, wd, radius, range, approximate, out);
  return 0;
}
