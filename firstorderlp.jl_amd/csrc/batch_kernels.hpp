// batch_kernels.hpp -- part of the single translation unit pdhg_hip.hip (included there, in order).
// One trial step for K LPs -- or K QPs with one objective matrix -- that share one constraint matrix
// (pdhg_batch_trial_step, abi_batch.hpp).
//
// x̄ and y' of the K members are kept MEMBER-INTERLEAVED in two batch buffers, X[j * Kp + k] and Y[i * Kp + k] (Kp = K
// rounded up to a power of two).  A group of Kp consecutive lanes owns one row of the product, lane k member k: the
// group reads each (column, value) entry once -- one address for all Kp lanes -- and gathers Kp * 8 contiguous bytes of
// X (64 B at K = 8, a 128-B line at K = 16) where the single-LP kernels gather 8 B of a line per member.
// Every lane adds its row strictly left to right from 0.0, like the single path's sequential rows (bit-exact with it for
// rows the single path sums sequentially: <= BLOCK_NNZ entries in strict order, <= RELAXED_MIN_ROW in relaxed order).
// Longer rows (more than BLOCK_NNZ entries in strict order, more than RELAXED_MIN_ROW in relaxed order) are cut into
// chunks of BATCH_CHUNK entries, each summed left to right, and the chunk sums added in a fixed order (strided by lane
// group, then the groups in order): within the relaxed bar, and no row is a latency chain of more than its chunk.  The step sums are Acc3 double-double
// partials rounded once at the end, so they come out as the single path's correctly rounded sums.
// Masked lanes (members not in the trial) issue no loads and no stores.
//
// A QP batch (pdhg_batch_set_objective_matrix) adds the two products of launch_primal / launch_q_interaction in the same
// form: the members' x are packed into X (batch_pack_kernel), Q X goes row by row into every member's qx (MODE_PLAIN: no
// sums), the primal step reads it and leaves x' - x interleaved in DX, and Q' DX is folded row by row into one
// double-double sum per member, dx . (Q' dx) (BATCH_MODE_QDX), which batch_final_kernel's QP form halves into out[4].
// The LP kernels are the instantiations they were: the QP forms are kernels of their own over the same bodies.
#pragma once

namespace {

constexpr int BATCH_MAX = 32;
constexpr int BATCH_CHUNK = 128;       // entries per chunk of a long row: 16 steps of one lane group
constexpr int BATCH_MAX_GRID = 4096;
constexpr int BATCH_U = 8;             // entries per lane and step: 8 gathers in flight

// What the batched kernels need of one member for one trial (pointers into the member's own handle).
struct BatchMemberDev {
  const double *x, *c, *aty, *lb, *ub, *y, *b;
  double *x_next, *sum_x, *y_next, *sum_y, *aty_next;
  double tau, theta, sigma, pend_w;
  int pend_x, pend_y, num_eq, pad;
};

struct BatchArgs {
  const BatchMemberDev *mem;   // [K]
  const int *act;              // [na] the active members, ascending
  unsigned act_mask;           // bit k: member k takes part in this trial
  int K, shift;                // Kp = 1 << shift
  double *X;                   // [n << shift] x̄, member-interleaved
  double *Y;                   // [m << shift] y', member-interleaved
};

__device__ __forceinline__ bool batch_lane_on(const BatchArgs &a, int k) { return k < a.K && ((a.act_mask >> k) & 1u); }

// Q' DX of a QP batch: batch_spmv_kernel's third product (beside MODE_PLAIN, MODE_DUAL, MODE_ATY of spmv_kernels.hpp)
enum { BATCH_MODE_QDX = 3 };
template <int MODE>
struct BatchNQ { static constexpr int value = MODE == BATCH_MODE_QDX ? 1 : ModeNQ<MODE>::value; };

// QP: x of every active member into X, where Q X gathers it (the primal step then overwrites it with x̄)
__global__ __launch_bounds__(TPB) void batch_pack_kernel(int n, BatchArgs a) {
  const int k = a.act[blockIdx.y];
  const double *x = a.mem[k].x;
  const int shift = a.shift;
  double *X = a.X;
  for (int j = blockIdx.x * TPB + threadIdx.x; j < n; j += gridDim.x * TPB) X[((size_t)j << shift) + k] = x[j];
}

// K1+K2 (+ the deferred K7) of every active member: the expressions of primal_kernel, element by element; x̄ goes to X.
// QP: with member k's Q x (qx[k]), and x' - x (diff_body's expression) goes to DX.
template <bool QP>
__device__ __forceinline__ void batch_primal_body(int n, BatchArgs a, double *const *qx, double *DX) {
  const int k = a.act[blockIdx.y];
  const BatchMemberDev &M = a.mem[k];
  const double *x = M.x, *c = M.c, *aty = M.aty, *lb = M.lb, *ub = M.ub;
  const double *q = QP ? qx[k] : nullptr;
  double *x_next = M.x_next, *sum_x = M.pend_x ? M.sum_x : nullptr;
  const double tau = M.tau, theta = M.theta, w = M.pend_w;
  const int shift = a.shift;
  double *X = a.X;
  for (int j = blockIdx.x * TPB + threadIdx.x; j < n; j += gridDim.x * TPB) {
    const double xv = x[j];
    if (sum_x) {
      const double t = xv * w;
      sum_x[j] = sum_x[j] + t;
    }
    double xn, xb;
    primal_one<QP, true>(xv, c[j], aty[j], QP ? q[j] : 0.0, lb[j], ub[j], tau, theta, xn, xb);
    x_next[j] = xn;
    X[((size_t)j << shift) + k] = xb;
    if (QP) DX[((size_t)j << shift) + k] = xn - xv;
  }
}
__global__ __launch_bounds__(TPB) void batch_primal_kernel(int n, BatchArgs a) { batch_primal_body<false>(n, a, nullptr, nullptr); }
__global__ __launch_bounds__(TPB) void batch_primal_qp_kernel(int n, BatchArgs a, double *const *qx, double *DX) {
  batch_primal_body<true>(n, a, qx, DX);
}

// Entries [rs, re) of one row against member k's column of the interleaved vector, left to right from 0.0.  The
// BATCH_U gathers of a step are requested back to back (their addresses need only the column loads), then added in
// order.
__device__ __forceinline__ double batch_row_sum(const int *__restrict__ col, const double *__restrict__ val, int rs, int re,
                                                const double *__restrict__ xin, int shift, int k) {
  double s = 0.0;
  int p = rs;
  for (; p + BATCH_U <= re; p += BATCH_U) {
    unsigned cc[BATCH_U];
    double v[BATCH_U], g[BATCH_U];
#pragma unroll
    for (int u = 0; u < BATCH_U; ++u) cc[u] = (unsigned)col[p + u];
#pragma unroll
    for (int u = 0; u < BATCH_U; ++u) v[u] = val[p + u];
    // the entries are in: an explicit vmcnt(0) here, where the wait-count pass would otherwise put waits between the
    // gathers below (it cannot tell the entry loads' registers from the gathers')
    __builtin_amdgcn_s_waitcnt(0x0F70);                 // vmcnt(0), expcnt / lgkmcnt untouched
#pragma unroll
    for (int u = 0; u < BATCH_U; ++u) g[u] = xin[((size_t)cc[u] << shift) + k];
    __builtin_amdgcn_sched_barrier(0);                  // all gathers issued before the first add
#pragma unroll
    for (int u = 0; u < BATCH_U; ++u) {
      const double t = v[u] * g[u];
      s = s + t;
    }
  }
  // the row's last cnt < BATCH_U entries as one more step with the loads of absent entries switched off: a short row
  // (most of a PageRank LP's) is two round trips, not two per entry.  (s never becomes -0.0 from +0.0, so skipping an
  // absent entry's add is the same as adding its 0.0: only the order of the real entries fixes the bits.)
  const int cnt = re - p;
  if (cnt > 0) {
    unsigned cc[BATCH_U - 1];
    double v[BATCH_U - 1], g[BATCH_U - 1];
#pragma unroll
    for (int u = 0; u < BATCH_U - 1; ++u) cc[u] = u < cnt ? (unsigned)col[p + u] : 0u;
#pragma unroll
    for (int u = 0; u < BATCH_U - 1; ++u) v[u] = u < cnt ? val[p + u] : 0.0;
    __builtin_amdgcn_s_waitcnt(0x0F70);                 // vmcnt(0), as above
#pragma unroll
    for (int u = 0; u < BATCH_U - 1; ++u) g[u] = u < cnt ? xin[((size_t)cc[u] << shift) + k] : 0.0;
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < BATCH_U - 1; ++u) {
      if (u < cnt) {
        const double t = v[u] * g[u];
        s = s + t;
      }
    }
  }
  return s;
}

// The fused epilogues of epi_apply for member k of the batch (MODE_DUAL: y', the pending sum_y, Y; MODE_ATY: A'y' and
// the three sums; MODE_PLAIN: the row sum into qx; BATCH_MODE_QDX: dot_kernel's product of the row sum and the row's dx).  BatchEpi holds the member's pointers and scalars in registers, read once per lane (the kernels'
// stores could alias the descriptor array, so reading them through it would reload them for every row); a row's
// operands are requested (batch_epi_load) before its sum, so that they arrive with the row's entries.
struct BatchEpi {
  const double *a, *b, *c;     // DUAL: y, b, sum_y (null: no pending update)   ATY: x', x, A'y   QDX: a = member k's DX
  double *out, *out2;          // DUAL: y', sum_y                              ATY: A'y'         PLAIN: out = qx
  double sigma, w;
  int num_eq;
};
template <int MODE>
__device__ __forceinline__ BatchEpi batch_epi(const BatchMemberDev &M) {
  BatchEpi e;
  if (MODE == MODE_DUAL) {
    e.a = M.y; e.b = M.b; e.c = M.pend_y ? M.sum_y : nullptr; e.out = M.y_next; e.out2 = M.sum_y;
    e.sigma = M.sigma; e.w = M.pend_w; e.num_eq = M.num_eq;
  } else {
    e.a = M.x_next; e.b = M.x; e.c = M.aty; e.out = M.aty_next; e.out2 = nullptr;
    e.sigma = 0.0; e.w = 0.0; e.num_eq = 0;
  }
  return e;
}
// the same for the two products of a QP batch: X is what the product gathers from (Q' DX: the launch passes DX)
template <int MODE>
__device__ __forceinline__ BatchEpi batch_q_epi(const double *X, int k, double *const *qx) {
  BatchEpi e;
  e.a = MODE == BATCH_MODE_QDX ? X + k : nullptr; e.b = e.c = nullptr;
  e.out = MODE == MODE_PLAIN ? qx[k] : nullptr; e.out2 = nullptr;
  e.sigma = 0.0; e.w = 0.0; e.num_eq = 0;
  return e;
}
template <int MODE>
__device__ __forceinline__ BatchEpi batch_epi_of(const BatchArgs &a, int k) { return batch_epi<MODE>(a.mem[k]); }
template <int MODE>
__device__ __forceinline__ BatchEpi batch_epi_of(const BatchArgs &a, int k, double *const *qx) { return batch_q_epi<MODE>(a.X, k, qx); }
template <int MODE>
__device__ __forceinline__ EpiOps batch_epi_load(const BatchEpi &e, int r, int shift) {
  EpiOps o;
  if (MODE == MODE_PLAIN) { o.a = o.b = o.c = 0.0; return o; }
  if (MODE == BATCH_MODE_QDX) { o.a = e.a[(size_t)r << shift]; o.b = o.c = 0.0; return o; }
  o.a = e.a[r];
  o.b = e.b[r];
  o.c = (MODE == MODE_ATY || e.c) ? e.c[r] : 0.0;
  return o;
}
template <int MODE>
__device__ __forceinline__ void batch_epilogue(const BatchArgs &a, const BatchEpi &e, int k, int r, double s, const EpiOps &o,
                                               Acc3 &acc) {
  if (MODE == MODE_PLAIN) {
    e.out[r] = s;
  } else if (MODE == BATCH_MODE_QDX) {
    dd_add(acc.hi[0], acc.lo[0], s * o.a);
  } else if (MODE == MODE_DUAL) {
    const double yo = o.a;
    if (e.c) {
      const double t = yo * e.w;
      e.out2[r] = o.c + t;
    }
    const double dg = o.b - s;
    const double t = e.sigma * dg;
    double yn = yo + t;
    if (r >= e.num_eq) yn = jl_max(yn, 0.0);
    e.out[r] = yn;
    a.Y[((size_t)r << a.shift) + k] = yn;
    const double dy = yn - yo;
    dd_add(acc.hi[0], acc.lo[0], dy * dy);
  } else {
    e.out[r] = s;
    const double dx = o.a - o.b;
    const double dd = s - o.c;
    dd_add(acc.hi[0], acc.lo[0], dx * dd);
    dd_add(acc.hi[1], acc.lo[1], dx * dx);
    dd_add(acc.hi[2], acc.lo[2], dd * dd);
  }
}

// Block partials of the NQ double-double sums, per member: lanes k, k + Kp, ... of a wave first (shuffles by multiples
// of Kp), then the four waves in order.  hi at part[(q * Kp + k) * slots + slot], lo NQ * Kp * slots further on.
template <int NQ>
__device__ __forceinline__ void batch_block_partials(Acc3 &acc, int shift, double *part, int slots, int slot) {
  if constexpr (NQ == 0) return;          // Q X: no sums
  __shared__ double red[2][NQ > 0 ? NQ : 1][TPB / WAVE][BATCH_MAX];
  const int Kp = 1 << shift;
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    double h = acc.hi[q], l = acc.lo[q];
    for (int off = WAVE / 2; off >= Kp; off >>= 1) {
      const double bh = __shfl_down(h, off, WAVE), bl = __shfl_down(l, off, WAVE);
      dd_add_dd(h, l, bh, bl);
    }
    if (lane < Kp) { red[0][q][wid][lane] = h; red[1][q][wid][lane] = l; }
  }
  __syncthreads();
  if ((int)threadIdx.x < Kp) {
    const int k = threadIdx.x;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      double h = 0.0, l = 0.0;
#pragma unroll
      for (int w = 0; w < TPB / WAVE; ++w) dd_add_dd(h, l, red[0][q][w][k], red[1][q][w][k]);
      const size_t at = ((size_t)q * Kp + k) * slots + slot;
      part[at] = h;
      part[(size_t)NQ * Kp * slots + at] = l;
    }
  }
}

// A X̄ with the dual epilogue (MODE_DUAL) or A' Y' with the A'y epilogue (MODE_ATY) over the rows of at most long_thr
// entries; a group of Kp lanes per row, rows dealt to the groups grid-stride.  QP batches: Q X into the members' qx
// (MODE_PLAIN) and dx . (Q' DX) (BATCH_MODE_QDX), both gathering from a.X (the second launch passes DX there).
// QX: nothing for the two products of A (the kernels every batch runs); `double *const *qx`, where the members' qx are,
// for the two products of a QP batch.
template <int MODE, typename... QX>
__global__ __launch_bounds__(TPB) void batch_spmv_kernel(int rows, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                         const double *__restrict__ val, int long_thr, BatchArgs a,
                                                         double *part, int slots, QX... qx) {
  const int shift = a.shift;
  const int k = threadIdx.x & ((1 << shift) - 1);
  const int grp = threadIdx.x >> shift, gpb = TPB >> shift;
  const bool on = batch_lane_on(a, k);
  const double *xin = MODE == MODE_ATY ? a.Y : a.X;
  Acc3 acc = acc3_zero();
  if (on) {
    const BatchEpi e = batch_epi_of<MODE>(a, k, qx...);
    for (int r = blockIdx.x * gpb + grp; r < rows; r += gridDim.x * gpb) {
      const int rs = rowptr[r], re = rowptr[r + 1];
      if (re - rs > long_thr) continue;              // batch_long_* kernels
      const EpiOps o = batch_epi_load<MODE>(e, r, shift);
      const double s = batch_row_sum(col, val, rs, re, xin, shift, k);
      batch_epilogue<MODE>(a, e, k, r, s, o, acc);
    }
  }
  batch_block_partials<BatchNQ<MODE>::value>(acc, shift, part, slots, blockIdx.x);
}

// Long rows, first half: chunk c = entries [chunks[c].x, chunks[c].y) of one long row, summed left to right per member.
__global__ __launch_bounds__(TPB) void batch_long_partial_kernel(int nchunks, const int2 *__restrict__ chunks,
                                                                 const int *__restrict__ col, const double *__restrict__ val,
                                                                 int use_y, BatchArgs a, double *__restrict__ cpart) {
  const int shift = a.shift;
  const int k = threadIdx.x & ((1 << shift) - 1);
  const int grp = threadIdx.x >> shift, gpb = TPB >> shift;
  if (!batch_lane_on(a, k)) return;
  const double *xin = use_y ? a.Y : a.X;
  for (int c = blockIdx.x * gpb + grp; c < nchunks; c += gridDim.x * gpb) {
    const int2 ch = chunks[c];
    cpart[((size_t)c << shift) + k] = batch_row_sum(col, val, ch.x, ch.y, xin, shift, k);
  }
}

// Long rows, second half: one workgroup per long row.  Group g of the Kp-lane groups adds the chunk sums g, g + gpb, ...
// of its member in order, then lane k adds the gpb group sums in group order (a fixed order), and runs the row's
// epilogue.  Block partials go to slots slot0 + blockIdx.x.
template <int MODE, typename... QX>
__global__ __launch_bounds__(TPB) void batch_long_final_kernel(int nlong, const int *__restrict__ long_row,
                                                               const int *__restrict__ long_cptr,
                                                               const double *__restrict__ cpart, BatchArgs a, double *part,
                                                               int slots, int slot0, QX... qx) {
  __shared__ double gsum[TPB];
  const int shift = a.shift;
  const int k = threadIdx.x & ((1 << shift) - 1);
  const int grp = threadIdx.x >> shift, gpb = TPB >> shift;
  const bool on = batch_lane_on(a, k);
  Acc3 acc = acc3_zero();
  for (int l = blockIdx.x; l < nlong; l += gridDim.x) {        // workgroup-uniform
    double s = 0.0;
    if (on)
      for (int c = long_cptr[l] + grp; c < long_cptr[l + 1]; c += gpb) s = s + cpart[((size_t)c << shift) + k];
    gsum[threadIdx.x] = s;
    __syncthreads();
    if ((int)threadIdx.x == k && on) {
      double t = 0.0;
      for (int g = 0; g < gpb; ++g) t = t + gsum[(g << shift) + k];
      const BatchEpi e = batch_epi_of<MODE>(a, k, qx...);
      batch_epilogue<MODE>(a, e, k, long_row[l], t, batch_epi_load<MODE>(e, long_row[l], shift), acc);
    }
    __syncthreads();
  }
  batch_block_partials<BatchNQ<MODE>::value>(acc, shift, part, slots, slot0 + blockIdx.x);
}

// Second stage, one workgroup per active member: the four sums of pdhg_trial_step's out[] from the block partials of
// the two products (out[0] dx.(A'y'-A'y), out[1] |dx|^2, out[2] |dy|^2, out[3] |A'y'-A'y|^2; out[4] = 0 for an LP).
// A QP batch (NS = 5): the fifth sum from the partials of Q' DX, rounded once and halved (abi_trial.hpp: out[4] = 0.5 * r[4]).
// PQ: nothing for an LP batch; (const double *pQ, int slotsQ) for a QP batch.
__device__ __forceinline__ const double *batch_pq_ptr() { return nullptr; }
__device__ __forceinline__ const double *batch_pq_ptr(const double *p, int) { return p; }
__device__ __forceinline__ int batch_pq_slots() { return 0; }
__device__ __forceinline__ int batch_pq_slots(const double *, int slots) { return slots; }
template <typename... PQ>
__global__ __launch_bounds__(TPB) void batch_final_kernel(BatchArgs a, const double *__restrict__ pA, int slotsA,
                                                          const double *__restrict__ pT, int slotsT, double *__restrict__ res,
                                                          PQ... pq) {
  constexpr int NS = sizeof...(PQ) > 0 ? 5 : 4;
  const double *pQ = batch_pq_ptr(pq...);
  const int slotsQ = batch_pq_slots(pq...);
  __shared__ double wh[NS][TPB / WAVE], wl[NS][TPB / WAVE];
  const int k = a.act[blockIdx.x];
  const int Kp = 1 << a.shift;
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  // (output, source): out[0] <- T q0, out[1] <- T q1, out[2] <- A q0, out[3] <- T q2, out[4] <- Q q0
  const double *hi[5] = {pT + (size_t)(0 * Kp + k) * slotsT, pT + (size_t)(1 * Kp + k) * slotsT,
                         pA + (size_t)k * slotsA, pT + (size_t)(2 * Kp + k) * slotsT, NS > 4 ? pQ + (size_t)k * slotsQ : nullptr};
  const size_t loff[5] = {(size_t)3 * Kp * slotsT, (size_t)3 * Kp * slotsT, (size_t)Kp * slotsA, (size_t)3 * Kp * slotsT,
                          (size_t)Kp * slotsQ};
  const int cnt[5] = {slotsT, slotsT, slotsA, slotsT, slotsQ};
#pragma unroll
  for (int o = 0; o < NS; ++o) {
    double h = 0.0, l = 0.0;
    for (int i = threadIdx.x; i < cnt[o]; i += TPB) dd_add_dd(h, l, hi[o][i], hi[o][loff[o] + i]);
    wave_sum_dd(h, l);
    if (lane == WAVE - 1) { wh[o][wid] = h; wl[o][wid] = l; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int o = 0; o < NS; ++o) {
      double h = 0.0, l = 0.0;
#pragma unroll
      for (int w = 0; w < TPB / WAVE; ++w) dd_add_dd(h, l, wh[o][w], wl[o][w]);
      const double r = h + l;
      res[5 * k + o] = o < 4 ? r : 0.5 * r;
    }
    if (NS == 4) res[5 * k + 4] = 0.0;
  }
}

// scale_problem's vector step (resc_apply_vectors_kernel's expressions) on one batch member's c, lb, ub, b
__global__ __launch_bounds__(TPB) void batch_scale_vectors_kernel(int n, int m, const double *__restrict__ dv,
                                                                  const double *__restrict__ ev, double *__restrict__ c,
                                                                  double *__restrict__ lb, double *__restrict__ ub,
                                                                  double *__restrict__ b) {
  const int tid = blockIdx.x * TPB + threadIdx.x, st = gridDim.x * TPB;
  for (int j = tid; j < n; j += st) {
    const double d = dv[j];
    c[j] = c[j] / d; ub[j] = ub[j] * d; lb[j] = lb[j] * d;
  }
  for (int i = tid; i < m; i += st) {
    const double e = ev[i];
    b[i] = b[i] / e;
  }
}

}  // namespace
