// batch_check_kernels.hpp -- part of the single translation unit pdhg_hip.hip (included there, after batch_resolve_kernels.hpp).
// A BATCH'S CHECKS in shared launches (abi_batch_checks.hpp, include/pdhg_hip_batch_checks.h).  Between two runs of
// batched trials every member of a batch asks for a termination evaluation and up to three rounds of trust-region
// problems, and each of those starts with A x, A' y (and Q x) at one of the member's points: K reads of the shared matrix
// per product where a trial reads it once.  Here the points of all asking members are packed member-interleaved
// (batch_check_pack_kernel) and one plain batched product per matrix (batch_spmv_kernel<MODE_PLAIN>, batch_kernels.hpp)
// writes every member's row sums into that member's own per-point cache; the evaluation's reductions run over
// (block, member) and one second-stage launch publishes every member's result words.
//
// Same bits as the per-member calls: the pack kernel's division is div_kernel's, a batched row sum is one lane adding left
// to right from 0.0 (the member's own order for rows without a long-row split), the evaluation kernels call the member
// kernels' own bodies (eval_rows_body / eval_cols_body / dist2_body) on the member's own grid and partials, and the second
// stage is final_quantities on multi_final_kernel's workgroup shape.
// Every kernel here is an ordinary launch: no grid barrier, nothing persistent.
#pragma once

namespace {

// One member's entry of a pass (a pass = one point kind): where its point is read from, whether the average has to be
// materialised first (do_div: src = the running sums, the quotient is also stored to avg_x / avg_y, as select_point's
// div_kernel launches store it), and whether the point goes into the interleaved vectors at lane k (pack).
struct BatchCheckPoint {
  const double *src_x, *src_y;
  double wx, wy;
  double *avg_x, *avg_y;
  int do_div, pack, k, pad;
};

// grid (blocks, entries).  Load side: consecutive lanes read consecutive elements of one member; the member-interleaved
// store is the strided side (batch_pack_kernel's shape).
__global__ __launch_bounds__(TPB) void batch_check_pack_kernel(int n, int m, const BatchCheckPoint *__restrict__ table,
                                                               double *__restrict__ X, double *__restrict__ Y, int shift) {
  const BatchCheckPoint p = table[blockIdx.y];
  const int tid = blockIdx.x * TPB + threadIdx.x, st = gridDim.x * TPB;
  const int k = p.k;
  if (p.do_div) {
    const double wx = p.wx, wy = p.wy;
    for (int j = tid; j < n; j += st) {
      const double v = p.src_x[j] / wx;
      p.avg_x[j] = v;
      if (p.pack) X[((size_t)j << shift) + k] = v;
    }
    for (int i = tid; i < m; i += st) {
      const double v = p.src_y[i] / wy;
      p.avg_y[i] = v;
      if (p.pack) Y[((size_t)i << shift) + k] = v;
    }
  } else if (p.pack) {
    for (int j = tid; j < n; j += st) X[((size_t)j << shift) + k] = p.src_x[j];
    for (int i = tid; i < m; i += st) Y[((size_t)i << shift) + k] = p.src_y[i];
  }
}

// ---- pdhg_eval_point's one-handle form for every carried member: grid (member's ev_grid, carried [, 3]) ----------------
// The table entry is the fleet's (FleetQpEvalArgs: the LP block and Q x at the point, nullptr for an LP).
__global__ __launch_bounds__(TPB) void batch_eval_rows_kernel(const FleetQpEvalArgs *__restrict__ table) {
  const FleetQpEvalArgs &a = table[blockIdx.y];
  eval_rows_body((int)blockIdx.x, (int)gridDim.x, a.m, a.ne, a.pt_ax, a.pt_y, a.E, a.b_o, a.partials, a.grid);
}

__global__ __launch_bounds__(TPB) void batch_eval_cols_kernel(const FleetQpEvalArgs *__restrict__ table) {
  const FleetQpEvalArgs &a = table[blockIdx.y];
  eval_cols_body((int)blockIdx.x, (int)gridDim.x, a.n, a.pt_aty, a.pt_qx, a.pt_x, a.Dv, a.c_o, a.lb_o, a.ub_o,
                 a.partials + (size_t)8 * a.grid, a.grid);
}

// blockIdx.z: 0 the average to the restart point (an empty average: the zeros of the member's memset), 1 the current
// iterate to the restart point, 2 the evaluated point's sums of squares
__global__ __launch_bounds__(TPB) void batch_eval_dist_kernel(const FleetQpEvalArgs *__restrict__ table) {
  const FleetQpEvalArgs &a = table[blockIdx.y];
  const int G = a.grid, z = (int)blockIdx.z;
  double *extra = a.partials + (size_t)22 * G + (size_t)2 * z * G;
  if (z == 0 && !a.have_avg) {               // (workgroup-uniform)
    if (threadIdx.x < 2) extra[threadIdx.x * G + blockIdx.x] = 0.0;
    return;
  }
  const double *xa = z == 0 ? a.avg_x : (z == 1 ? a.x : a.pt_x), *ya = z == 0 ? a.avg_y : (z == 1 ? a.y : a.pt_y);
  const double *xb = z == 2 ? nullptr : a.x_r, *yb = z == 2 ? nullptr : a.y_r;
  dist2_body((int)blockIdx.x, (int)gridDim.x, a.n, a.m, xa, xb, ya, yb, extra, G);
}

// Second stage, one workgroup per carried member (multi_final_kernel's shape: the same lane-to-partial assignment, tree and
// max mask), which publishes the member's 28 result words into the member's block of the batch's pinned array.
__global__ __launch_bounds__(FINAL_TPB) void batch_eval_final_kernel(const FleetQpEvalArgs *__restrict__ table) {
  const FleetQpEvalArgs &a = table[blockIdx.x];
  __shared__ double res[EV_HOST_SLOTS];
  final_quantities(a.partials, a.grid, a.grid, 28, 0, EVAL_MAX_MASK, FINAL_TPB / WAVE, a.scal, res);
  __syncthreads();
  if (threadIdx.x == 0) publish_words(a.host_out, EV_HOST_SLOTS, 28, a.seq, [&](int q) { return res[q]; });
}

// What one call uploads, once: the passes' entries, the output tables of the batched products ([pass][A x, A' y, Q x]
// [member]: the members' per-point cache buffers) and the evaluation's table.
struct BatchCheckStage {
  BatchCheckPoint pts[3][BATCH_MAX];
  double *out[3][3][BATCH_MAX];
  FleetQpEvalArgs ev[BATCH_MAX];
};

}  // namespace
