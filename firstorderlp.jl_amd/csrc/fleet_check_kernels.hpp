// fleet_check_kernels.hpp -- part of the single translation unit pdhg_hip.hip (included there, after small_lp_kernel.hpp).
// A FLEET'S CHECKS in shared launches (host_checks.hpp, abi_fleet_checks.hpp): between two batches of steps every
// member of a fleet asks for a termination evaluation and up to five trust-region problems.  Per member that is about a
// dozen launches of a few microseconds of work each and up to four trips to the host, the members taking them in turn.
// Here one workgroup does one member's (or one problem's) work, and a launch carries one workgroup per item: the item is
// an entry of a table in device memory (small_lp_fleet_kernel's pattern), the workgroups share nothing.
//
// Same bits as the per-member calls.  Every kernel here calls the per-member kernels' own bodies: a row's products are
// added left to right from 0.0 (small_row_sum: what launch_spmv<MODE_PLAIN> gives for rows of up to SMALL_MAX_ROW entries
// in both row orders -- longer rows keep a member out), the evaluation's ev_grid blocks run one after the other as
// virtual blocks through eval_rows_body / eval_cols_body / dist2_body, their partials go through multi_final_kernel's
// per-quantity routine (final_quantities), and a trust-region problem is tr_small_body.
//
// Small QPs (PDHG_SMALL_QP=1) ride in launches of kernels of their own names (fleet_qp_*) beside the LPs', from tables of
// their own blocks: the LP kernels' text with Q x at the point as one more row sum per column, handed to eval_cols_body
// and (by the host, TrSmallArgs::qx) to tr_small_body.  The QP kernels restate the LP kernels' statements instead of
// sharing a __device__ body with them: routed through an inlined body the LP kernels compile to the same IR but to another
// register assignment and order of address computations, and the LP kernels are to stay the instructions they were.
#pragma once

namespace {

// ---- A x and A' y at one point of one member (select_point + point_products of one handle) -------------------------
struct FleetPointArgs {
  int n, m;
  int do_div, do_products;                   // materialise the average first / compute the products
  CsrView A, T;                              // CSR(A) (m rows), CSR(A') (n rows)
  const double *sum_x, *sum_y;               // do_div: px = sum_x / wx, py = sum_y / wy (div_kernel's arithmetic)
  double wx, wy;
  double *avg_x, *avg_y;
  const double *px, *py;                     // the point
  double *ax, *aty;                          // the member's per-point cache buffers
};

__global__ __launch_bounds__(TPB) void fleet_point_products_kernel(const FleetPointArgs *__restrict__ table, int count) {
  if ((int)blockIdx.x >= count) return;
  const FleetPointArgs a = table[blockIdx.x];
  const int tid = threadIdx.x;
  if (a.do_div) {
    for (int j = tid; j < a.n; j += TPB) a.avg_x[j] = a.sum_x[j] / a.wx;
    for (int i = tid; i < a.m; i += TPB) a.avg_y[i] = a.sum_y[i] / a.wy;
    __syncthreads();                         // (workgroup-scope release / acquire: the rows below read what other threads wrote)
  }
  if (!a.do_products) return;
  for (int r = tid; r < a.m; r += TPB) a.ax[r] = small_row_sum(a.A, r, a.px);
  for (int j = tid; j < a.n; j += TPB) a.aty[j] = small_row_sum(a.T, j, a.py);
}

// The QP form: the LP block, CSR(Q) and where Q x goes.  (A block of its own: the LP kernel's table keeps its stride.)
struct FleetQpPointArgs : FleetPointArgs {
  CsrView Q;                                 // CSR(Q) (n rows)
  double *qx;                                // the member's per-point cache buffer of Q x
};

__global__ __launch_bounds__(TPB) void fleet_qp_point_products_kernel(const FleetQpPointArgs *__restrict__ table, int count) {
  if ((int)blockIdx.x >= count) return;
  const FleetQpPointArgs a = table[blockIdx.x];
  const int tid = threadIdx.x;
  if (a.do_div) {
    for (int j = tid; j < a.n; j += TPB) a.avg_x[j] = a.sum_x[j] / a.wx;
    for (int i = tid; i < a.m; i += TPB) a.avg_y[i] = a.sum_y[i] / a.wy;
    __syncthreads();                         // (as above: Q x reads the point as the rows of A do)
  }
  if (!a.do_products) return;
  for (int r = tid; r < a.m; r += TPB) a.ax[r] = small_row_sum(a.A, r, a.px);
  for (int j = tid; j < a.n; j += TPB) a.aty[j] = small_row_sum(a.T, j, a.py);
  // launch_spmv<MODE_PLAIN, 2>(h, h->Q, ...)'s order for rows of up to SMALL_MAX_ROW entries: what point_products runs
  for (int j = tid; j < a.n; j += TPB) a.qx[j] = small_row_sum(a.Q, j, a.px);
}

// ---- pdhg_eval_point's one-handle form for one member, in one workgroup -----------------------------------------------
// eval_rows_kernel, eval_cols_kernel, three dist2_kernel launches (or the zeros of an empty average) and
// multi_final_kernel: the member's `grid` blocks as virtual blocks, block after block into the member's own partials,
// then the second stage of all 28 quantities and the member's own result words.
struct FleetEvalArgs {
  int n, m, ne, grid, have_avg;
  const double *pt_x, *pt_y, *pt_ax, *pt_aty;               // the evaluated point and its products
  const double *E, *b_o, *Dv, *c_o, *lb_o, *ub_o;           // the original problem
  const double *avg_x, *avg_y, *x, *y, *x_r, *y_r;          // the distances' operands
  double *partials;                                          // [EV_MAXQ * grid]
  double *scal;                                              // where multi_final_kernel leaves the totals on the device
  double *host_out;
  unsigned long long seq;
};
constexpr unsigned EVAL_MAX_MASK = 0xF0u | (0x7Fu << 15);   // quantities 4-7 and 15-21 are maxima (pdhg_eval_point)

__global__ __launch_bounds__(TPB) void fleet_eval_kernel(const FleetEvalArgs *__restrict__ table, int count) {
  if ((int)blockIdx.x >= count) return;
  const FleetEvalArgs a = table[blockIdx.x];
  __shared__ double res[EV_HOST_SLOTS];
  const int G = a.grid;
  double *extra = a.partials + (size_t)22 * G;
  for (int vb = 0; vb < G; ++vb) {
    eval_rows_body(vb, G, a.m, a.ne, a.pt_ax, a.pt_y, a.E, a.b_o, a.partials, G);
    __syncthreads();                         // (the block reductions share their staging words from one virtual block to the next)
    eval_cols_body(vb, G, a.n, a.pt_aty, nullptr, a.pt_x, a.Dv, a.c_o, a.lb_o, a.ub_o, a.partials + (size_t)8 * G, G);
    __syncthreads();
    if (a.have_avg) {
      dist2_body(vb, G, a.n, a.m, a.avg_x, a.x_r, a.avg_y, a.y_r, extra, G);
      __syncthreads();
    } else if (threadIdx.x < 2) {
      extra[threadIdx.x * G + vb] = 0.0;     // the memset of an empty average
    }
    dist2_body(vb, G, a.n, a.m, a.x, a.x_r, a.y, a.y_r, extra + (size_t)2 * G, G);
    __syncthreads();
    dist2_body(vb, G, a.n, a.m, a.pt_x, nullptr, a.pt_y, nullptr, extra + (size_t)4 * G, G);
    __syncthreads();
  }
  // (the barrier above is also the release of every partial to the waves that read them now)
  final_quantities(a.partials, G, G, 28, 0, EVAL_MAX_MASK, TPB / WAVE, a.scal, res);
  __syncthreads();
  if (threadIdx.x == 0) publish_words(a.host_out, EV_HOST_SLOTS, 28, a.seq, [&](int q) { return res[q]; });
}

// The QP form: fleet_eval_kernel with Q x at the evaluated point handed to eval_cols_body (x'Qx and |Qx|inf of the unscaled
// point, quantities 14 and 21) where the LP kernel hands nullptr.
struct FleetQpEvalArgs : FleetEvalArgs {
  const double *pt_qx;
};

__global__ __launch_bounds__(TPB) void fleet_qp_eval_kernel(const FleetQpEvalArgs *__restrict__ table, int count) {
  if ((int)blockIdx.x >= count) return;
  const FleetQpEvalArgs a = table[blockIdx.x];
  __shared__ double res[EV_HOST_SLOTS];
  const int G = a.grid;
  double *extra = a.partials + (size_t)22 * G;
  for (int vb = 0; vb < G; ++vb) {
    eval_rows_body(vb, G, a.m, a.ne, a.pt_ax, a.pt_y, a.E, a.b_o, a.partials, G);
    __syncthreads();
    eval_cols_body(vb, G, a.n, a.pt_aty, a.pt_qx, a.pt_x, a.Dv, a.c_o, a.lb_o, a.ub_o, a.partials + (size_t)8 * G, G);
    __syncthreads();
    if (a.have_avg) {
      dist2_body(vb, G, a.n, a.m, a.avg_x, a.x_r, a.avg_y, a.y_r, extra, G);
      __syncthreads();
    } else if (threadIdx.x < 2) {
      extra[threadIdx.x * G + vb] = 0.0;
    }
    dist2_body(vb, G, a.n, a.m, a.x, a.x_r, a.y, a.y_r, extra + (size_t)2 * G, G);
    __syncthreads();
    dist2_body(vb, G, a.n, a.m, a.pt_x, nullptr, a.pt_y, nullptr, extra + (size_t)4 * G, G);
    __syncthreads();
  }
  final_quantities(a.partials, G, G, 28, 0, EVAL_MAX_MASK, TPB / WAVE, a.scal, res);
  __syncthreads();
  if (threadIdx.x == 0) publish_words(a.host_out, EV_HOST_SLOTS, 28, a.seq, [&](int q) { return res[q]; });
}

// ---- one trust-region problem per workgroup (tr_small_kernel's body) ---------------------------------------------------
// The launch's dynamic LDS is that of its largest item; a smaller one uses the front of it.
__global__ __launch_bounds__(TRS_TPB) void fleet_tr_kernel(const TrSmallArgs *__restrict__ table, int count) {
  if ((int)blockIdx.x >= count) return;
  const TrSmallArgs a = table[blockIdx.x];
  tr_small_body(a);
}

}  // namespace
