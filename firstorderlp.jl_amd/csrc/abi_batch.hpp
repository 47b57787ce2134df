// abi_batch.hpp -- part of the single translation unit pdhg_hip.hip (included there, inside its extern "C" block).
// C ABI: batched solves of K LPs -- or K QPs with one objective matrix -- that share one constraint matrix
// (batch_kernels.hpp holds the kernels).
//
// A batch is a pdhg_handle that owns the matrix and its layouts (built once, as pdhg_create builds them) and K member
// handles.  A member is an ordinary pdhg_handle with its own vectors whose A / At BORROW the batch's layouts (`owner`
// set): every single-LP entry point works on it unchanged, on the batch's stream; pdhg_destroy skips it and the batch
// frees it.  The persistent one-launch trial (trial_kernel.hpp) keeps per-layout counters, so it stays off on members
// and on the batch handle; the other launch paths give the same bits.
// pdhg_batch_set_objective_matrix makes the batch a QP batch: Q / Qt are built on the batch handle and lent to the members
// the same way (the batch frees them, destroy_shard leaves a member's alone), every member gets its own qx and tmp_n2.

// one of the products of a batched trial: A X̄ (dual epilogue), A' Y' (A'y epilogue); a QP batch: Q X and Q' DX as well
struct BatchProduct {
  int rows = 0, grid = 0, slots = 0, long_thr = 0;
  int nlong = 0, nchunks = 0, long_grid = 0, chunk_grid = 0;
  int *long_row = nullptr, *long_cptr = nullptr;
  int2 *chunks = nullptr;
  double *cpart = nullptr;   // [nchunks << shift]
  double *part = nullptr;    // [2 * NQ * Kp * slots] double-double block partials
};

struct BatchState {
  int K = 0, shift = 0;
  std::vector<pdhg_handle *> mem;
  BatchProduct PA, PT;
  double *X = nullptr, *Y = nullptr;
  // a QP batch (the batch handle's has_q): Q X (no sums, no partials), Q' DX, x' - x member-interleaved like X, and where
  // the members' qx are (qx_dev[k])
  BatchProduct PQ, PQt;
  double *DX = nullptr;
  double **qx_dev = nullptr;
  BatchMemberDev *mdev = nullptr, *mhost = nullptr;
  int *act_dev = nullptr, *act_host = nullptr;
  double *res_dev = nullptr, *res_host = nullptr;
  int64_t trials = 0;
  // re-solves (abi_batch_resolve.hpp): what the calls did (`other`: whether the last warm start ran the batched product)
  ResolveCounters rsv;
  // the checks in shared launches (abi_batch_checks.hpp), allocated by the first such call: what a call uploads (device copy,
  // pinned staging, "the upload has been read"), the members' result words (BATCH_MAX x (EV_HOST_SLOTS + 2), pinned) and
  // their sequence number, and pdhg_batch_check_info's counters 0-4 and 7 (5 and 6 are counted where a member answers:
  // pdhg_handle::bchk_*)
  struct Checks {
    BatchCheckStage *stage_dev = nullptr, *stage_host = nullptr;
    hipEvent_t uploaded = nullptr;
    bool upload_pending = false;
    double *res = nullptr;
    unsigned long long seq = 0;
    int64_t calls = 0, batched = 0, own = 0, cached = 0, carried = 0, launches = 0;
  } chk;
};

static void batch_free_product(BatchProduct &P) {
  for (void *p : {(void *)P.long_row, (void *)P.long_cptr, (void *)P.chunks, (void *)P.cpart, (void *)P.part})
    if (p) (void)hipFree(p);
  P = BatchProduct{};
}

// Back to an LP batch: the members give their borrowed copies of Q / Qt back (they keep qx and tmp_n2), the batch frees
// the layouts and what the two Q products needed.  The stream is idle.
static void batch_drop_q(pdhg_handle *h) {
  BatchState &B = *h->bat;
  for (pdhg_handle *m : B.mem) {
    m->Q = CsrDev(); m->Qt = CsrDev();
    m->has_q = false;
  }
  free_csr_dev(h->Q); free_csr_dev(h->Qt);
  h->has_q = false;
  batch_free_product(B.PQ);
  batch_free_product(B.PQt);
  if (B.DX) (void)hipFree(B.DX);
  if (B.qx_dev) (void)hipFree(B.qx_dev);
  B.DX = nullptr; B.qx_dev = nullptr;
}

static void batch_release(pdhg_handle *h) {
  BatchState *B = h->bat;
  if (!B) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  batch_drop_q(h);
  for (pdhg_handle *m : B->mem) destroy_shard(m);
  batch_free_product(B->PA);
  batch_free_product(B->PT);
  for (void *p : {(void *)B->X, (void *)B->Y, (void *)B->mdev, (void *)B->act_dev, (void *)B->res_dev})
    if (p) (void)hipFree(p);
  for (void *p : {(void *)B->mhost, (void *)B->act_host, (void *)B->res_host, (void *)B->chk.stage_host, (void *)B->chk.res})
    if (p) (void)hipHostFree(p);
  if (B->chk.stage_dev) (void)hipFree(B->chk.stage_dev);
  if (B->chk.uploaded) (void)hipEventDestroy(B->chk.uploaded);
  delete B;
  h->bat = nullptr;
}

// A member: the batch's matrix layouts (struct copies: the same device arrays), its own vectors -- what create_shard
// allocates for a plain handle (alloc_shard_vectors).
static int batch_create_member(pdhg_handle *o, const double *c, const double *b, const double *lb, const double *ub,
                               pdhg_handle **out) {
  *out = nullptr;
  pdhg_handle *h = new pdhg_handle();
  h->self = h;
  h->owner = o;
  h->device = o->device;
  h->stream = o->stream; h->own_stream = false;
  h->m = o->m; h->n = o->n; h->nnz = o->nnz; h->num_eq = o->num_eq;
  h->cn = o->n; h->n_alloc = o->n; h->m_global = o->m;
  h->remap = o->remap; h->relaxed = o->relaxed; h->lazy_accept = o->lazy_accept;
  h->A = o->A; h->At = o->At;
  h->coop_mode = 0;
  if (int rc = alloc_shard_vectors(h, c, b, lb, ub)) { destroy_shard(h); return rc; }
  *out = h;
  return 0;
}

// Long rows of one product (host row pointers of the device CSR) and its launch geometry.
static int batch_build_product(BatchProduct &P, const CsrDev &D, int shift, int long_thr) {
  P.rows = D.rows;
  P.long_thr = long_thr;
  std::vector<int> rp((size_t)D.rows + 1, 0);
  if (D.rows > 0) HIP_TRY(hipMemcpy(rp.data(), D.rowptr, sizeof(int) * rp.size(), hipMemcpyDeviceToHost));
  std::vector<int> lrow, lcptr(1, 0);
  std::vector<int2> ch;
  for (int r = 0; r < D.rows; ++r) {
    if (rp[(size_t)r + 1] - rp[(size_t)r] <= long_thr) continue;
    lrow.push_back(r);
    for (int s = rp[(size_t)r]; s < rp[(size_t)r + 1]; s += BATCH_CHUNK) ch.push_back(make_int2(s, std::min(s + BATCH_CHUNK, rp[(size_t)r + 1])));
    lcptr.push_back((int)ch.size());
  }
  const int gpb = TPB >> shift;
  P.grid = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)D.rows + gpb - 1) / gpb, BATCH_MAX_GRID));
  P.nlong = (int)lrow.size();
  P.nchunks = (int)ch.size();
  if (P.nlong > 0) {
    P.long_grid = std::min(P.nlong, BATCH_MAX_GRID);
    P.chunk_grid = std::min((P.nchunks + gpb - 1) / gpb, BATCH_MAX_GRID);
    HIP_TRY(hipMalloc((void **)&P.long_row, sizeof(int) * lrow.size()));
    HIP_TRY(hipMalloc((void **)&P.long_cptr, sizeof(int) * lcptr.size()));
    HIP_TRY(hipMalloc((void **)&P.chunks, sizeof(int2) * ch.size()));
    HIP_TRY(hipMemcpy(P.long_row, lrow.data(), sizeof(int) * lrow.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(P.long_cptr, lcptr.data(), sizeof(int) * lcptr.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(P.chunks, ch.data(), sizeof(int2) * ch.size(), hipMemcpyHostToDevice));
    int rc = alloc_zero(&P.cpart, (int64_t)P.nchunks << shift);
    if (rc) return rc;
  }
  P.slots = P.grid + P.long_grid;
  return 0;
}

static pdhg_handle *batch_of(pdhg_handle *h) { return (h && h->bat) ? h : nullptr; }

// apply_scaling's vector step on every member of a batch (pdhg_rescale on the batch handle)
static int batch_scale_members(pdhg_handle *h, const double *dv, const double *ev) {
  for (pdhg_handle *m : h->bat->mem) {
    hipLaunchKernelGGL(batch_scale_vectors_kernel, dim3(h->ew_grid_nm), dim3(TPB), 0, h->stream, (int)h->n, (int)h->m, dv, ev,
                       m->c, m->lb, m->ub, m->b);
    HIP_TRY(hipGetLastError());
    if (int rcb = bounds_rebuild(m)) return rcb;
    m->state_version += 1;
    m->matrix_version += 1;
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int pdhg_create_batch(pdhg_handle **out, int count, int64_t m, int64_t n, int64_t nnz, const int64_t *colptr,
                      const int64_t *rowval, const double *nzval, int index_base, const double *c, const double *b,
                      const double *lb, const double *ub, int64_t num_equalities, int device_id, void *stream) {
  if (!out) return fail(-1, "out == NULL");
  *out = nullptr;
  if (count < 1 || count > BATCH_MAX) return fail(-1, "pdhg_create_batch: count must be 1.." + std::to_string(BATCH_MAX));
  if (!c || !lb || !ub || (m > 0 && !b)) return fail(-1, "null input array");
  int64_t cap = (int64_t)INT32_MAX - 1;
  if (const char *ev = getenv("PDHG_MAX_SHARD_NNZ")) cap = std::max<int64_t>(1, atoll(ev));
  if (nnz > cap) return fail(-2, "pdhg_create_batch: a batch's matrix must index its nonzeros with 32 bits (no row segments)");
  pdhg_handle *h = nullptr;
  int rc = create_shard(&h, m, n, nnz, colptr, rowval, nzval, index_base, c, b, lb, ub, num_equalities, device_id, stream, n, 0);
  if (rc) return rc;
  h->coop_mode = 0;
  BatchState *B = new BatchState();
  h->bat = B;
  B->K = count;
  while ((1 << B->shift) < count) ++B->shift;
#define CKB(expr) do { int _rc = (expr); if (_rc) { batch_release(h); destroy_shard(h); return _rc; } } while (0)
  for (int k = 0; k < count; ++k) {
    pdhg_handle *mb = nullptr;
    CKB(batch_create_member(h, c + (size_t)k * n, b ? b + (size_t)k * m : nullptr, lb + (size_t)k * n, ub + (size_t)k * n, &mb));
    B->mem.push_back(mb);
  }
  // rows the single path sums one lane left to right stay whole (bit-exact with it); longer ones are chunked
  const int long_thr = h->relaxed ? RELAXED_MIN_ROW : BLOCK_NNZ;
  CKB(batch_build_product(B->PA, h->A, B->shift, long_thr));
  CKB(batch_build_product(B->PT, h->At, B->shift, long_thr));
  const int64_t Kp = (int64_t)1 << B->shift;
  CKB(alloc_zero(&B->X, n * Kp));
  CKB(alloc_zero(&B->Y, m * Kp));
  CKB(alloc_zero(&B->PA.part, 2 * Kp * B->PA.slots));
  CKB(alloc_zero(&B->PT.part, 6 * Kp * B->PT.slots));
  CKB(alloc_zero(&B->res_dev, 5 * BATCH_MAX));
  auto hip = [](hipError_t e, const char *what) { return e == hipSuccess ? 0 : fail_hip(e, what); };
  CKB(hip(hipMalloc((void **)&B->mdev, sizeof(BatchMemberDev) * BATCH_MAX), "hipMalloc (batch)"));
  CKB(hip(hipMalloc((void **)&B->act_dev, sizeof(int) * BATCH_MAX), "hipMalloc (batch)"));
  CKB(hip(hipHostMalloc((void **)&B->mhost, sizeof(BatchMemberDev) * BATCH_MAX, hipHostMallocDefault), "hipHostMalloc (batch)"));
  CKB(hip(hipHostMalloc((void **)&B->act_host, sizeof(int) * BATCH_MAX, hipHostMallocDefault), "hipHostMalloc (batch)"));
  CKB(hip(hipHostMalloc((void **)&B->res_host, sizeof(double) * 5 * BATCH_MAX, hipHostMallocDefault), "hipHostMalloc (batch)"));
  CKB(hip(hipDeviceSynchronize(), "hipDeviceSynchronize (batch)"));
#undef CKB
  // The batch handle itself runs no iterations: its iterate, average and scratch vectors go (the layouts were tuned with
  // them above).  It keeps c, b, lb, ub, which pdhg_rescale's scaling pass updates with the cumulative factors; every
  // other single-LP entry point refuses it (check_handle) -- they run on the members.
  for (double **v : {&h->x, &h->x_next, &h->xbar, &h->y, &h->y_next, &h->aty, &h->aty_next, &h->sum_x, &h->sum_y, &h->tmp_n,
                     &h->tmp_m}) {
    if (*v) (void)hipFree(*v);
    *v = nullptr;
  }
  *out = h;
  return 0;
}

/* The objective matrix of every member (CSC like pdhg_set_objective_matrix's): the batch becomes a QP batch, or -- when
 * every stored value is 0.0 -- an LP batch again.  May be called at any time between trials; the members keep their iterates. */
int pdhg_batch_set_objective_matrix(pdhg_handle *batch, int64_t q_nnz, const int64_t *q_colptr, const int64_t *q_rowval,
                                    const double *q_nzval, int index_base) {
  if (!batch_of(batch)) return fail(-1, "pdhg_batch_set_objective_matrix: not a batch handle");
  if (int rcw = batch_awaits_rescale(batch, "pdhg_batch_set_objective_matrix: ")) return rcw;
  if (q_nnz < 0 || !q_colptr || (q_nnz > 0 && (!q_rowval || !q_nzval))) return fail(-1, "null input array");
  pdhg_handle *h = batch;
  BatchState &B = *h->bat;
  bool all_zero = true;
  for (int64_t k = 0; k < q_nnz; ++k) if (q_nzval[k] != 0.0) all_zero = false;
  std::vector<int> t_rowptr, rowptr;
  ivec t_col, col;
  dvec t_val, val;
  int rc = 0;
  if (!all_zero) {
    rc = csc_to_both(h->n, h->n, q_nnz, q_colptr, q_rowval, q_nzval, index_base, t_rowptr, t_col, t_val, rowptr, col, val);
    if (rc) return rc;
  }
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  batch_drop_q(h);
  h->state_version += 1; h->matrix_version += 1;
  h->csc_ascending = -1;               // (pdhg_batch_update_matrix_values looks at the new Q's columns too)
  for (pdhg_handle *m : B.mem) {
    // the launch paths were decided for the problem without (or with another) Q: decide again at the next trial
    // (the persistent one-launch trial stays off on a member: coop_mode is 0)
    m->graph_mode = -1;
    m->small_lp_mode = -1;
    graph_destroy(m->tgraph[0]); graph_destroy(m->tgraph[1]);
    m->state_version += 1; m->matrix_version += 1;
  }
  if (all_zero) return 0;          // iszero(objective_matrix): LP path (pdhg.jl:536)
  auto build = [&]() -> int {
    int r2;
    if ((r2 = build_csr_dev(h->Q, (int)h->n, (int)h->n, rowptr, col, val, h->remap))) return r2;
    if ((r2 = build_csr_dev(h->Qt, (int)h->n, (int)h->n, t_rowptr, t_col, t_val, h->remap))) return r2;
    const int long_thr = h->relaxed ? RELAXED_MIN_ROW : BLOCK_NNZ;
    if ((r2 = batch_build_product(B.PQ, h->Q, B.shift, long_thr))) return r2;
    if ((r2 = batch_build_product(B.PQt, h->Qt, B.shift, long_thr))) return r2;
    const int64_t Kp = (int64_t)1 << B.shift;
    if ((r2 = alloc_zero(&B.PQt.part, 2 * Kp * B.PQt.slots))) return r2;
    if ((r2 = alloc_zero(&B.DX, h->n * Kp))) return r2;
    double *qx[BATCH_MAX] = {};
    for (int k = 0; k < B.K; ++k) {
      pdhg_handle *m = B.mem[(size_t)k];
      if (!m->qx && (r2 = alloc_zero(&m->qx, m->n))) return r2;
      if (!m->tmp_n2 && (r2 = alloc_zero(&m->tmp_n2, m->n))) return r2;
      qx[k] = m->qx;
    }
    HIP_TRY(hipMalloc((void **)&B.qx_dev, sizeof(double *) * BATCH_MAX));
    HIP_TRY(hipMemcpy(B.qx_dev, qx, sizeof(double *) * BATCH_MAX, hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    return 0;
  };
  if ((rc = build())) { batch_drop_q(h); return rc; }
  h->has_q = true;
  for (pdhg_handle *m : B.mem) {   // struct copies: the same device arrays (pdhg_rescale scales them in place)
    m->Q = h->Q; m->Qt = h->Qt;
    m->has_q = true;
  }
  return 0;
}

int pdhg_batch_member(pdhg_handle *batch, int k, pdhg_handle **member) {
  if (!member) return fail(-1, "member == NULL");
  *member = nullptr;
  if (!batch_of(batch)) return fail(-1, "pdhg_batch_member: not a batch handle");
  if (k < 0 || k >= batch->bat->K) return fail(-1, "pdhg_batch_member: member index out of range");
  *member = batch->bat->mem[(size_t)k];
  return 0;
}

// One trial of every active member; out[5 k .. 5 k + 4] = what pdhg_trial_step returns for member k.
static int batch_trial(pdhg_handle *h, const double *step_size, const double *primal_weight, double theta, const int *active,
                       double *out) {
  BatchState &B = *h->bat;
  int na = 0;
  unsigned mask = 0;
  for (int k = 0; k < B.K; ++k) {
    if (!active[k]) continue;
    pdhg_handle *m = B.mem[(size_t)k];
    BatchMemberDev &d = B.mhost[k];
    d.x = m->x; d.c = m->c; d.aty = m->aty; d.lb = m->lb; d.ub = m->ub; d.y = m->y; d.b = m->b;
    d.x_next = m->x_next; d.sum_x = m->sum_x; d.y_next = m->y_next; d.sum_y = m->sum_y; d.aty_next = m->aty_next;
    d.tau = step_size[k] / primal_weight[k];
    d.theta = theta;
    d.sigma = primal_weight[k] * step_size[k];
    d.pend_w = m->pend_w;
    d.pend_x = m->pend_x ? 1 : 0; d.pend_y = m->pend_y ? 1 : 0;
    d.num_eq = (int)m->num_eq; d.pad = 0;
    B.act_host[na++] = k;
    mask |= 1u << k;
  }
  if (na == 0) return 0;
  RoctxRange roctx_range("pdhg_batch_trial_step");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpyAsync(B.mdev, B.mhost, sizeof(BatchMemberDev) * (size_t)B.K, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(B.act_dev, B.act_host, sizeof(int) * (size_t)na, hipMemcpyHostToDevice, h->stream));
  BatchArgs a{B.mdev, B.act_dev, mask, B.K, B.shift, B.X, B.Y};
  const int n = (int)h->n, m = (int)h->m;
  const bool qp = h->has_q;
  // Q X into the members' qx or dx . (Q' DX) into P.part, from what aq.X holds: the short rows, then the long-row pair
  auto q_product = [&](const CsrDev &D, BatchProduct &P, bool qdx, const BatchArgs &aq) {
    if (qdx) hipLaunchKernelGGL((batch_spmv_kernel<BATCH_MODE_QDX, double *const *>), dim3(P.grid), dim3(TPB), 0, h->stream, P.rows,
                                D.rowptr, D.col, D.val, P.long_thr, aq, P.part, P.slots, (double *const *)B.qx_dev);
    else hipLaunchKernelGGL((batch_spmv_kernel<MODE_PLAIN, double *const *>), dim3(P.grid), dim3(TPB), 0, h->stream, P.rows, D.rowptr,
                            D.col, D.val, P.long_thr, aq, P.part, P.slots, (double *const *)B.qx_dev);
    if (P.nlong == 0) return;
    hipLaunchKernelGGL(batch_long_partial_kernel, dim3(P.chunk_grid), dim3(TPB), 0, h->stream, P.nchunks, (const int2 *)P.chunks,
                       (const int *)D.col, (const double *)D.val, 0, aq, P.cpart);
    if (qdx) hipLaunchKernelGGL((batch_long_final_kernel<BATCH_MODE_QDX, double *const *>), dim3(P.long_grid), dim3(TPB), 0, h->stream,
                                P.nlong, (const int *)P.long_row, (const int *)P.long_cptr, (const double *)P.cpart, aq, P.part,
                                P.slots, P.grid, (double *const *)B.qx_dev);
    else hipLaunchKernelGGL((batch_long_final_kernel<MODE_PLAIN, double *const *>), dim3(P.long_grid), dim3(TPB), 0, h->stream,
                            P.nlong, (const int *)P.long_row, (const int *)P.long_cptr, (const double *)P.cpart, aq, P.part,
                            P.slots, P.grid, (double *const *)B.qx_dev);
  };
  if (qp) {       // launch_primal's Q x, recomputed on every trial like there
    hipLaunchKernelGGL(batch_pack_kernel, dim3(ew_grid(n), na), dim3(TPB), 0, h->stream, n, a);
    q_product(h->Q, B.PQ, false, a);
    hipLaunchKernelGGL(batch_primal_qp_kernel, dim3(ew_grid(n), na), dim3(TPB), 0, h->stream, n, a, (double *const *)B.qx_dev, B.DX);
  } else {
    hipLaunchKernelGGL(batch_primal_kernel, dim3(ew_grid(n), na), dim3(TPB), 0, h->stream, n, a);
  }
  auto product = [&](const CsrDev &D, BatchProduct &P, bool dual) {
    if (dual) hipLaunchKernelGGL(batch_spmv_kernel<MODE_DUAL>, dim3(P.grid), dim3(TPB), 0, h->stream, P.rows, D.rowptr, D.col, D.val,
                                 P.long_thr, a, P.part, P.slots);
    else hipLaunchKernelGGL(batch_spmv_kernel<MODE_ATY>, dim3(P.grid), dim3(TPB), 0, h->stream, P.rows, D.rowptr, D.col, D.val,
                            P.long_thr, a, P.part, P.slots);
    if (P.nlong == 0) return;
    hipLaunchKernelGGL(batch_long_partial_kernel, dim3(P.chunk_grid), dim3(TPB), 0, h->stream, P.nchunks, (const int2 *)P.chunks,
                       (const int *)D.col, (const double *)D.val, dual ? 0 : 1, a, P.cpart);
    if (dual) hipLaunchKernelGGL(batch_long_final_kernel<MODE_DUAL>, dim3(P.long_grid), dim3(TPB), 0, h->stream, P.nlong,
                                 (const int *)P.long_row, (const int *)P.long_cptr, (const double *)P.cpart, a, P.part, P.slots, P.grid);
    else hipLaunchKernelGGL(batch_long_final_kernel<MODE_ATY>, dim3(P.long_grid), dim3(TPB), 0, h->stream, P.nlong,
                            (const int *)P.long_row, (const int *)P.long_cptr, (const double *)P.cpart, a, P.part, P.slots, P.grid);
  };
  if (m > 0) product(h->A, B.PA, true);
  if (n > 0) product(h->At, B.PT, false);
  if (qp) {       // launch_q_interaction's Q' dx and its dot with dx
    BatchArgs aq = a;
    aq.X = B.DX;
    q_product(h->Qt, B.PQt, true, aq);
    hipLaunchKernelGGL((batch_final_kernel<const double *, int>), dim3(na), dim3(TPB), 0, h->stream, a, (const double *)B.PA.part,
                       m > 0 ? B.PA.slots : 0, (const double *)B.PT.part, n > 0 ? B.PT.slots : 0, B.res_dev,
                       (const double *)B.PQt.part, B.PQt.slots);
  } else {
    hipLaunchKernelGGL(batch_final_kernel<>, dim3(na), dim3(TPB), 0, h->stream, a, (const double *)B.PA.part, m > 0 ? B.PA.slots : 0,
                       (const double *)B.PT.part, n > 0 ? B.PT.slots : 0, B.res_dev);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(B.res_host, B.res_dev, sizeof(double) * 5 * (size_t)B.K, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int i = 0; i < na; ++i) {
    const int k = B.act_host[i];
    pdhg_handle *mb = B.mem[(size_t)k];
    mb->pend_x = mb->pend_y = false;     // the deferred K7 rode on this trial's kernels
    for (int q = 0; q < 5; ++q) out[5 * k + q] = B.res_host[5 * k + q];
  }
  B.trials += 1;
  return 0;
}

int pdhg_batch_trial_step(pdhg_handle *batch, const double *step_size, const double *primal_weight, double theta,
                          const int *active, double *out) {
  if (!batch_of(batch)) return fail(-1, "pdhg_batch_trial_step: not a batch handle");
  if (int rcw = batch_awaits_rescale(batch, "pdhg_batch_trial_step: ")) return rcw;
  if (!step_size || !primal_weight || !active || !out) return fail(-1, "null argument");
  return batch_trial(batch, step_size, primal_weight, theta, active, out);
}

int pdhg_batch_accept(pdhg_handle *batch, const int *accept, const double *avg_weight) {
  if (!batch_of(batch)) return fail(-1, "pdhg_batch_accept: not a batch handle");
  if (int rcw = batch_awaits_rescale(batch, "pdhg_batch_accept: ")) return rcw;
  if (!accept || !avg_weight) return fail(-1, "null argument");
  for (int k = 0; k < batch->bat->K; ++k) {
    if (!accept[k]) continue;
    const int rc = pdhg_accept(batch->bat->mem[(size_t)k], avg_weight[k]);
    if (rc) return rc;
  }
  return 0;
}

/* n_steps take_steps of every active member in lockstep: a member that rejects its trial keeps trialling (the members that
 * have accepted in this step are masked), the step-size rule per member is adaptive_step_rule with the host's pow, the
 * accept's weight is the member's step size on entry.  A member that raises numerical_error stops after that step (it is
 * counted in steps_done, as pdhg_take_steps_adaptive counts it) and takes no further trials. */
int pdhg_batch_take_steps_adaptive(pdhg_handle *batch, int64_t n_steps, double reduction_exponent, double growth_exponent,
                                   double *step_size, const double *primal_weight, int64_t *total_number_iterations,
                                   double *cumulative_kkt_passes, int *numerical_error, const int *active,
                                   int64_t *steps_done) {
  RoctxRange roctx_range("pdhg_batch_take_steps_adaptive");
  if (!batch_of(batch)) return fail(-1, "pdhg_batch_take_steps_adaptive: not a batch handle");
  if (int rcw = batch_awaits_rescale(batch, "pdhg_batch_take_steps_adaptive: ")) return rcw;
  if (!step_size || !primal_weight || !total_number_iterations || !cumulative_kkt_passes || !numerical_error || !active ||
      !steps_done)
    return fail(-1, "null argument");
  if (n_steps < 0) return fail(-2, "pdhg_batch_take_steps_adaptive: n_steps < 0");
  const int K = batch->bat->K;
  int live[BATCH_MAX], need[BATCH_MAX], acc[BATCH_MAX];
  double entry[BATCH_MAX], raw[5 * BATCH_MAX];
  for (int k = 0; k < K; ++k) {
    live[k] = active[k] ? 1 : 0;
    if (live[k]) { numerical_error[k] = 0; steps_done[k] = 0; }
  }
  for (int64_t s = 0; s < n_steps; ++s) {
    int any = 0;
    for (int k = 0; k < K; ++k) { need[k] = live[k]; entry[k] = step_size[k]; any |= live[k]; }
    if (!any) break;
    for (;;) {
      int pending = 0;
      for (int k = 0; k < K; ++k) {
        acc[k] = 0;
        if (need[k]) { total_number_iterations[k] += 1; pending = 1; }
      }
      if (!pending) break;
      int rc = batch_trial(batch, step_size, primal_weight, 1.0, need, raw);
      if (rc) return rc;
      for (int k = 0; k < K; ++k) {
        if (!need[k]) continue;
        StepIO io{step_size[k], total_number_iterations[k], cumulative_kkt_passes[k], numerical_error[k], steps_done[k],
                  primal_weight[k], reduction_exponent, growth_exponent};
        const StepRule rule = step_after_trial(io, raw + 5 * k);
        if (rule.numerical_error) live[k] = 0;
        else acc[k] = rule.accept;
        if (rule.numerical_error || rule.accept) {       // the take_step is over (a failing one counts as taken)
          need[k] = 0;
          io.steps_done += 1;
        }
      }
      if ((rc = pdhg_batch_accept(batch, acc, entry))) return rc;
    }
  }
  return 0;
}
