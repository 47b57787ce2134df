// fleet_rescale_kernels.hpp -- part of the single translation unit pdhg_hip.hip (included there, after resolve_kernels.hpp).
// A FLEET'S RESCALING in one shared launch (abi_fleet_rescale.hpp, include/pdhg_hip_fleet_rescale.h).  pdhg_rescale of a
// small member is about a dozen launches per step, each a few microseconds of work, a view rebuild per step and eight
// allocations, the members taking them in turn.  Here one workgroup takes one member through every step of
// rescale_problem and through pdhg_matrix_max_abs, and a launch carries one workgroup per member: the member is an entry
// of a table in device memory (fleet_point_products_kernel's pattern), the workgroups share nothing.
//
// Same bits as the member's own pdhg_rescale + pdhg_matrix_max_abs.  A row statistic is row_op_kernel's row body
// (row_op_row: one wave per row, lanes stride the row by 64, the same shuffle tree, the same pow in this translation
// unit), the workgroup's waves taking rows wave, wave + nwaves, ...; a scaled entry is scale_csr_kernel's row body; every
// elementwise statement is the resc_* / resolve_record kernels' element body, in pdhg_rescale's order.  max |a| is a
// maximum of absolute values: any order gives the same bits.
//
// The step's factor vectors live in LDS -- dv | ev, their inverses, the L2 step's scales (the QP Ruiz step's column
// maxima of Q), the call's cumulative factors: four vectors of n + m doubles, dynamic LDS sized per launch.  The matrix
// values stay in global memory: between the phases of a step they are written and then read by other waves of the same
// workgroup, ordered by __syncthreads() (a workgroup barrier with workgroup-scope release / acquire).
#pragma once

namespace {

constexpr int FRS_TPB = 512;      // 8 waves: rows of a 27 x 32 member four deep per wave; two waves per SIMD keep the VGPR budget of pow

// the steps of a call, the same for every member
struct FleetRescaleSteps {
  int ruiz, l2, pock;
  double alpha;
};

struct FleetRescaleArgs {
  int n, m, has_q, retained;
  CsrView A, T, Q, Qt;                       // CSR(A) (m rows), CSR(A') (n rows); QP: CSR(Q), CSR(Q') (n rows each)
  double *a_val, *t_val, *q_val, *qt_val;    // ... and their values, to be scaled in place
  int64_t t_nnz;
  double *c, *lb, *ub, *b;
  double *rec;                               // retained: where the call's first step goes in the record, step-major
  double *rcum_d, *rcum_e;                   // retained: the handle's running products
  double *out;                               // [n + m + 1]: variable_rescaling, constraint_rescaling, max |a|
};

template <int OP>
__device__ __forceinline__ void frs_row_op(const CsrView &A, int cols, double pexp, const double *inv_scale, double *out) {
  const int lane = threadIdx.x & (WAVE - 1);
  for (int r = threadIdx.x / WAVE; r < A.rows; r += FRS_TPB / WAVE)
    row_op_row<OP>(A, r, A.rowptr[r], A.rowptr[r + 1], lane, cols, pexp, inv_scale, out);
}
__device__ __forceinline__ void frs_scale(const CsrView &A, double *val, const double *inv_e, const double *inv_d, int transposed) {
  const int lane = threadIdx.x & (WAVE - 1);
  for (int r = threadIdx.x / WAVE; r < A.rows; r += FRS_TPB / WAVE)
    scale_csr_row(r, A.rowptr[r], A.rowptr[r + 1], lane, A.col, val, inv_e, inv_d, transposed);
}

// apply_scaling of one step whose factors stand in dv | ev: the inverses, the vectors, the cumulative factors, the
// retained record (step `s` of the call), then every copy of the matrices.  Ends behind a barrier.
__device__ __forceinline__ void frs_apply(const FleetRescaleArgs &a, int s, double *fac, double *inv, double *cum) {
  const int n = a.n, m = a.m, tid = threadIdx.x;
  double *dv = fac, *ev = fac + n, *inv_d = inv, *inv_e = inv + n;
  for (int i = tid; i < m; i += FRS_TPB) resc_zero_to_one_inv_elem(ev, inv_e, i, 0);
  for (int j = tid; j < n; j += FRS_TPB) resc_zero_to_one_inv_elem(dv, inv_d, j, 0);
  for (int j = tid; j < n; j += FRS_TPB) resc_apply_col(dv[j], a.c, a.lb, a.ub, cum, j);
  for (int i = tid; i < m; i += FRS_TPB) resc_apply_row(ev[i], a.b, cum + n, i);
  if (a.retained) {
    double *rec_step = a.rec + (int64_t)s * ((int64_t)n + m);
    for (int j = tid; j < n; j += FRS_TPB) resolve_record_col(dv[j], rec_step, a.rcum_d, j);
    for (int i = tid; i < m; i += FRS_TPB) resolve_record_row(ev[i], rec_step, a.rcum_e, n, i);
  }
  __syncthreads();                           // the inverses are complete
  frs_scale(a.A, a.a_val, inv_e, inv_d, 0);
  frs_scale(a.T, a.t_val, inv_e, inv_d, 1);
  if (a.has_q) {                             // (D^-1 Q) D^-1 on CSR(Q) and, entry by entry, on CSR(Q')
    frs_scale(a.Q, a.q_val, inv_d, inv_d, 0);
    frs_scale(a.Qt, a.qt_val, inv_d, inv_d, 1);
  }
  __syncthreads();                           // the next statistic reads the values other waves scaled
}

__global__ __launch_bounds__(FRS_TPB) void fleet_rescale_kernel(const FleetRescaleArgs *__restrict__ table, int count,
                                                                FleetRescaleSteps st) {
  extern __shared__ double frs_lds[];
  __shared__ double red[FRS_TPB / WAVE];
  if ((int)blockIdx.x >= count) return;
  const FleetRescaleArgs a = table[blockIdx.x];
  const int n = a.n, m = a.m, tid = threadIdx.x, len = n + m;
  double *fac = frs_lds, *inv = frs_lds + len, *tmp = frs_lds + 2 * len, *cum = frs_lds + 3 * len;
  double *dv = fac, *ev = fac + n, *inv_d = inv, *inv_e = inv + n, *tmp_d = tmp, *tmp_e = tmp + n;
  for (int k = tid; k < len; k += FRS_TPB) cum[k] = 1.0;
  __syncthreads();
  int s = 0;
  // ruiz_rescaling, p = Inf: sqrt of the row / column max |a| (QP: columns over [A; Q]), zeros -> 1
  for (int it = 0; it < st.ruiz; ++it, ++s) {
    frs_row_op<ROP_MAXABS>(a.T, m, 0.0, nullptr, dv);
    frs_row_op<ROP_MAXABS>(a.A, n, 0.0, nullptr, ev);
    if (a.has_q) frs_row_op<ROP_MAXABS>(a.Qt, n, 0.0, nullptr, tmp_d);
    __syncthreads();
    if (a.has_q)
      for (int j = tid; j < n; j += FRS_TPB) dv[j] = resc_max_elem(dv[j], tmp_d[j]);
    for (int j = tid; j < n; j += FRS_TPB) dv[j] = resc_sqrt_elem(dv[j]);
    for (int i = tid; i < m; i += FRS_TPB) ev[i] = resc_sqrt_elem(ev[i]);
    frs_apply(a, s, fac, inv, cum);
  }
  // l2_norm_rescaling: sqrt of the row / column L2 norms, each taken as scale * sqrt(sum (a / scale)^2), zeros -> 1
  if (st.l2) {
    frs_row_op<ROP_MAXABS>(a.T, m, 0.0, nullptr, tmp_d);
    frs_row_op<ROP_MAXABS>(a.A, n, 0.0, nullptr, tmp_e);
    __syncthreads();
    for (int j = tid; j < n; j += FRS_TPB) resc_zero_to_one_inv_elem(tmp_d, inv_d, j, 1);
    for (int i = tid; i < m; i += FRS_TPB) resc_zero_to_one_inv_elem(tmp_e, inv_e, i, 1);
    __syncthreads();
    frs_row_op<ROP_SUMSQ_SCALED>(a.T, m, 0.0, inv_d, dv);
    frs_row_op<ROP_SUMSQ_SCALED>(a.A, n, 0.0, inv_e, ev);
    __syncthreads();
    for (int j = tid; j < n; j += FRS_TPB) dv[j] = resc_sqrt_elem(resc_l2norm_elem(tmp_d[j], dv[j]));
    for (int i = tid; i < m; i += FRS_TPB) ev[i] = resc_sqrt_elem(resc_l2norm_elem(tmp_e[i], ev[i]));
    frs_apply(a, s, fac, inv, cum);
    ++s;
  }
  // pock_chambolle_rescaling: sqrt of sum |a|^(2 - alpha) over a column, of sum |a|^alpha over a row
  if (st.pock) {
    frs_row_op<ROP_SUMPOW>(a.T, m, 2.0 - st.alpha, nullptr, dv);
    frs_row_op<ROP_SUMPOW>(a.A, n, st.alpha, nullptr, ev);
    __syncthreads();
    for (int j = tid; j < n; j += FRS_TPB) dv[j] = resc_sqrt_elem(dv[j]);
    for (int i = tid; i < m; i += FRS_TPB) ev[i] = resc_sqrt_elem(ev[i]);
    frs_apply(a, s, fac, inv, cum);
    ++s;
  }
  // the call's cumulative factors, and pdhg_matrix_max_abs: max |a| over CSR(A')'s values
  for (int j = tid; j < n; j += FRS_TPB) a.out[j] = cum[j];
  for (int i = tid; i < m; i += FRS_TPB) a.out[n + i] = cum[n + i];
  double mx = 0.0;
  for (int64_t k = tid; k < a.t_nnz; k += FRS_TPB) mx = fmax(mx, fabs(a.t_val[k]));
  mx = wave_max(mx);
  if ((tid & (WAVE - 1)) == 0) red[tid / WAVE] = mx;
  __syncthreads();
  if (tid == 0) {
    double t = red[0];
    for (int w = 1; w < FRS_TPB / WAVE; ++w) t = fmax(t, red[w]);
    a.out[len] = t;
  }
}

}  // namespace
