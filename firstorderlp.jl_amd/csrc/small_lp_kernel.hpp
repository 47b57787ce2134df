// small_lp_kernel.hpp -- part of the single translation unit pdhg_hip.hip (included there, after trial_kernel.hpp).
// SMALL LPs (n, m up to ~1400: the class of the reference's Netlib runs, BASELINE configs[1]): a batch of adaptive
// take_steps (pdhg.jl:653-731; pdhg_take_steps_adaptive) in ONE workgroup with every vector in LDS.
//
// Why a kernel of its own.  For an LP of a few thousand nonzeros a trial is nothing but latency: one launch per trial
// costs ~28 us whatever the size (launch, two grid barriers, the completion ticket, the result's trip to the host), and
// walking the row blocks of the stream layout in one workgroup does not help either (a phase is a chain of ~5 dependent
// trips to memory, ~7 us per row block: profiles/r03_trial_kernel.txt).  Here nothing leaves the compute unit between
// two trials: x, x', xbar, A'y, A'y', c, the bounds, sum_x (n each) and y, y', b, sum_y (m each) live in LDS, the
// matrix (static, a few hundred KB at most) streams from the L1 / L2, one thread owns one row, and the step rule
// (adaptive_step_rule, the host loop's own function) runs on thread 0.  A trial is three phases between
// __syncthreads: ~3 us instead of ~28.
//
// Same bits as every other path: the phases restate the element arithmetic of primal_one / row_epilogue verbatim
// (separate multiply and add, -ffp-contract=off), a row's products are added left to right as the stream kernel adds
// rows of up to 256 entries in either row order (longer rows make the LP ineligible), and the three sums are
// double-double (exactly rounded whatever the grouping).  tests/test_gpu_small_lp.py: bitwise against one launch per
// trial and against the oracle.
//
// The two other step-size policies (pdhg.jl:555-647, 737-767; pdhg_take_steps_constant / _malitsky_pock) run in the same
// body, chosen by a template argument: the same LDS footprint, thread-count rule, write-back and result words, the same
// element arithmetic.  Constant: three phases per step and nothing else -- no sums, no block reduction, no rule (every
// trial is accepted), the averages take step_size at every step.  Malitsky-Pock: x' once per take_step with the step
// size on entry, then up to 60 dual trials (xbar with the ratio as extrapolation coefficient, the dual half, A'y', two
// double-double sums, malitsky_pock_rule on thread 0).  Their launches end between take_steps only.
// tests/test_gpu_step_policies.py: bitwise against the host loops in C and in Python, and against the oracle.
//
// SMALL QPs (PDHG_SMALL_QP=1; MPC horizons, QP nodes of a branch and bound): the same body in its QP form, a third template
// argument, behind kernels of their own names (small_qp_*; the LP instantiations above keep theirs and compile to what
// they were).  A QP step is the LP step plus Q x in the gradient, Q' dx and one more double-double sum
// (pdhg.jl:536-541, saddle_point.jl:1093-1100; launch_primal / launch_q_interaction on the per-launch path): two more
// n-vectors in LDS (qx, dx: 11n + 4m doubles), Q and Q' streamed row by row like A and A'.  qx = Q x is computed at the
// start of the launch and after every accept (x does not move on a rejection, so the per-launch path's product of every
// trial has the same bits); dx . (Q' dx) does not depend on y' and rides on the dual phase, reduced together with dy^2
// (two quantities there, three in the A'y' phase: block_sum_dd holds three).  The constant policy needs qx alone;
// Malitsky-Pock refuses QPs (pdhg.jl, policy_handle_check).  tests/test_gpu_small_qp.py: bitwise against one launch per
// trial and against the oracle.
#pragma once

#include <type_traits>

namespace {

constexpr int SMALL_TPB = 1024;          // threads of the workgroup for n or m beyond SMALL_FEW_ROWS; 256 below (fewer waves per barrier)
constexpr int SMALL_FEW_ROWS = 256;      // (30 x 30: 173k it/s with 256 threads against 126k with 1024; 300 x 300: 116k against 120k)
constexpr int SMALL_MAX_ROW = 256;       // rows of more entries are summed wave-parallel in relaxed order elsewhere

struct SmallLpArgs {
  int n, m, num_eq;
  CsrView A, T;                           // CSR(A) (m rows), CSR(A') (n rows)
  double *x, *y, *aty, *sum_x, *sum_y;    // read at the start, written back at the end
  const double *c, *lb, *ub, *b;
  double primal_weight, step_size;
  int n_steps, max_trials, table_len;
  int pend;                               // an accept before this launch left its average update pending
  double pend_w;
  double wsum_x, wsum_y;
  const double *pow_red, *pow_growth;
  volatile double *res_host;
  unsigned long long seq;
  // Malitsky-Pock alone: ratio_step_sizes on entry and the policy's three parameters
  double ratio, downscaling_factor, breaking_factor, interpolation_coefficient;
};

// The QP form's block: the LP fields and both copies of the objective matrix.  (A block of its own: the LP kernels'
// argument segment and their fleet table's stride stay what they were.)
struct SmallQpArgs : SmallLpArgs {
  CsrView Q, Qt;                          // CSR(Q), CSR(Q') (n rows each)
};

// one row's sum: products added strictly left to right, eight entries requested at a time
__device__ __forceinline__ double small_row_sum(const CsrView &M, int r, const double *xs) {
  int k = M.rowptr[r];
  const int ke = M.rowptr[r + 1];
  double s = 0.0;
  for (; k + 8 <= ke; k += 8) {
    int ci[8];
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { ci[u] = M.col[k + u]; v[u] = M.val[k + u]; }
#pragma unroll
    for (int u = 0; u < 8; ++u) { const double p = v[u] * xs[ci[u]]; s = s + p; }
  }
  for (; k < ke; ++k) { const double p = M.val[k] * xs[M.col[k]]; s = s + p; }
  return s;
}

// The whole launch of one LP: what a workgroup does with one argument block, whoever handed it over -- the solo kernel
// (the block by value) or the fleet kernel (its entry of a table in device memory).
template <int THREADS, int POLICY = SMALL_ADAPTIVE, bool QP = false>
__device__ __forceinline__ void small_lp_steps_body(const std::conditional_t<QP, SmallQpArgs, SmallLpArgs> &a) {
  static_assert(!(QP && POLICY == SMALL_MALITSKY_POCK), "Malitsky and Pock linesearch is only supported for LPs");
  extern __shared__ double lds[];
  __shared__ double red[6][THREADS / WAVE];
  __shared__ double s_dec[3];
  __shared__ double s_st[5];              // step size of the trial, step size on entry, (Malitsky-Pock: the ratio), weight sums x / y
  const int n = a.n, m = a.m, tid = threadIdx.x;
  double *xs = lds, *xn = xs + n, *xb = xn + n, *at = xb + n, *atn = at + n;
  double *cs = atn + n, *lbs = cs + n, *ubs = lbs + n, *sx = ubs + n;
  double *ys = sx + n, *yn = ys + m, *bs = yn + m, *sy = bs + m;
  [[maybe_unused]] double *qx = sy + m, *dxs = qx + n;       // QP form alone: Q x of the iterate, x' - x of the trial
  for (int j = tid; j < n; j += THREADS) {
    xs[j] = a.x[j]; at[j] = a.aty[j]; cs[j] = a.c[j]; lbs[j] = a.lb[j]; ubs[j] = a.ub[j]; sx[j] = a.sum_x[j];
  }
  for (int r = tid; r < m; r += THREADS) { ys[r] = a.y[r]; bs[r] = a.b[r]; sy[r] = a.sum_y[r]; }
  if (tid == 0) {
    s_st[0] = a.step_size; s_st[1] = a.step_size; s_st[3] = a.wsum_x; s_st[4] = a.wsum_y;
    if constexpr (POLICY == SMALL_MALITSKY_POCK) s_st[2] = a.ratio;
  }
  __syncthreads();
  if (a.pend) {                           // the deferred K7 of the accept before this launch (saddle_point.jl:252-301)
    for (int j = tid; j < n; j += THREADS) { const double t = xs[j] * a.pend_w; sx[j] = sx[j] + t; }
    for (int r = tid; r < m; r += THREADS) { const double t = ys[r] * a.pend_w; sy[r] = sy[r] + t; }
  }
  if constexpr (QP) {                     // qx = Q x (launch_primal's product): one thread per row, left to right
    for (int j = tid; j < n; j += THREADS) qx[j] = small_row_sum(a.Q, j, xs);
    __syncthreads();
  }
  int steps = 0, trials = 0, num_err = 0, mid = 0;
  if constexpr (POLICY == SMALL_ADAPTIVE) {
    while (steps < a.n_steps && (trials < a.max_trials || mid) && trials < a.table_len) {
      const double step = s_st[0];
      const double tau = step / a.primal_weight, sigma = a.primal_weight * step;
      double pw_r = 0.0, pw_g = 0.0;
      if (tid == 0) { pw_r = a.pow_red[trials]; pw_g = a.pow_growth[trials]; }
      // ---- K1 + K2: x' = proj(x - tau (c - A'y)), xbar = x' + (x' - x)        (primal_one, vector_kernels.hpp)
      for (int j = tid; j < n; j += THREADS) {
        double v, b2;
        if constexpr (QP) {
          primal_one<true, true>(xs[j], cs[j], at[j], qx[j], lbs[j], ubs[j], tau, 1.0, v, b2);
          dxs[j] = v - xs[j];                         // (diff_body)
        } else {
          primal_one<false, true>(xs[j], cs[j], at[j], 0.0, lbs[j], ubs[j], tau, 1.0, v, b2);
        }
        xn[j] = v; xb[j] = b2;
      }
      __syncthreads();
      // ---- K3 + K4: y' = proj(y + sigma (b - A xbar)), sum dy^2                 (row_epilogue<MODE_DUAL>)
      Acc3 acc = acc3_zero();
      if constexpr (QP) {                             // dx . (Q' dx): launch_q_interaction's product and dot_body's sum
        for (int j = tid; j < n; j += THREADS) {
          const double s = small_row_sum(a.Qt, j, dxs);
          dd_add(acc.hi[1], acc.lo[1], s * dxs[j]);
        }
      }
      for (int r = tid; r < m; r += THREADS) {
        const double s = small_row_sum(a.A, r, xb);
        const double yo = ys[r];
        const double dg = bs[r] - s;
        const double t = sigma * dg;
        double v = yo + t;
        if (r >= a.num_eq) v = jl_max(v, 0.0);
        yn[r] = v;
        const double dy = v - yo;
        dd_add(acc.hi[0], acc.lo[0], dy * dy);
      }
      block_sum_dd<QP ? 2 : 1, THREADS>(acc, red);  // (ends with the totals on thread 0; a barrier inside)
      const double dy2 = acc.hi[0] + acc.lo[0];
      [[maybe_unused]] const double dxqdx = acc.hi[1] + acc.lo[1];
      __syncthreads();
      // ---- K5 + K6: A'y' and the interaction sums                                  (row_epilogue<MODE_ATY>)
      Acc3 acc3 = acc3_zero();
      for (int j = tid; j < n; j += THREADS) {
        const double s = small_row_sum(a.T, j, yn);
        atn[j] = s;
        const double dx = xn[j] - xs[j];
        const double dd = s - at[j];
        dd_add(acc3.hi[0], acc3.lo[0], dx * dd);
        dd_add(acc3.hi[1], acc3.lo[1], dx * dx);
        dd_add(acc3.hi[2], acc3.lo[2], dd * dd);
      }
      block_sum_dd<3, THREADS>(acc3, red);
      if (tid == 0) {
        double raw[5];
        raw[0] = acc3.hi[0] + acc3.lo[0]; raw[1] = acc3.hi[1] + acc3.lo[1]; raw[2] = dy2; raw[3] = acc3.hi[2] + acc3.lo[2];
        raw[4] = QP ? 0.5 * dxqdx : 0.0;
        const StepRule rule = adaptive_step_rule(raw, a.primal_weight, step, pw_r, pw_g);
        s_dec[0] = (double)rule.accept; s_dec[1] = (double)rule.numerical_error; s_dec[2] = rule.next_step;
      }
      __syncthreads();
      const int nerr = __builtin_amdgcn_readfirstlane((int)(s_dec[1] != 0.0));
      const int acc_ok = __builtin_amdgcn_readfirstlane((int)(s_dec[0] != 0.0));
      trials += 1;
      if (nerr) { num_err = 1; mid = 0; break; }
      mid = !acc_ok;
      if (acc_ok) {
        // update_solution_in_solver_state (pdhg.jl:496-525): the trial point becomes the iterate; the averages take it
        // with the step size on entry as weight
        double *t0 = xs; xs = xn; xn = t0;
        double *t1 = ys; ys = yn; yn = t1;
        double *t2 = at; at = atn; atn = t2;
        const double wgt = s_st[1];
        for (int j = tid; j < n; j += THREADS) { const double t = xs[j] * wgt; sx[j] = sx[j] + t; }
        for (int r = tid; r < m; r += THREADS) { const double t = ys[r] * wgt; sy[r] = sy[r] + t; }
        if constexpr (QP) {                           // Q x of the new iterate (every thread has finished reading xn)
          for (int j = tid; j < n; j += THREADS) qx[j] = small_row_sum(a.Q, j, xs);
        }
        steps += 1;
      }
      __syncthreads();
      if (tid == 0) {
        const double next = s_dec[2];
        if (acc_ok) {
          const double entry = s_st[1];
          s_st[3] = s_st[3] + entry; s_st[4] = s_st[4] + entry;
          s_st[1] = next;
        }
        s_st[0] = next;
      }
      __syncthreads();
    }
  }
  if constexpr (POLICY == SMALL_CONSTANT) {
    // take_step(::ConstantStepsizeParams) (pdhg.jl:737-767): one trial with theta = 1, accepted whatever it gives; the
    // averages take step_size.  The accept's sums ride on the phases that write their element: sum_y on the dual half,
    // sum_x on A'y' (thread j wrote x'[j] itself in the first phase).
    const double step = a.step_size;
    const double tau = step / a.primal_weight, sigma = a.primal_weight * step;
    double wx = a.wsum_x, wy = a.wsum_y;
    for (; steps < a.n_steps; ++steps) {
      for (int j = tid; j < n; j += THREADS) {
        double v, b2;
        if constexpr (QP) primal_one<true, true>(xs[j], cs[j], at[j], qx[j], lbs[j], ubs[j], tau, 1.0, v, b2);
        else primal_one<false, true>(xs[j], cs[j], at[j], 0.0, lbs[j], ubs[j], tau, 1.0, v, b2);
        xn[j] = v; xb[j] = b2;
      }
      __syncthreads();
      for (int r = tid; r < m; r += THREADS) {
        const double s = small_row_sum(a.A, r, xb);
        const double dg = bs[r] - s;
        const double t = sigma * dg;
        double v = ys[r] + t;
        if (r >= a.num_eq) v = jl_max(v, 0.0);
        yn[r] = v;
        const double w = v * step;
        sy[r] = sy[r] + w;
      }
      __syncthreads();
      for (int j = tid; j < n; j += THREADS) {
        atn[j] = small_row_sum(a.T, j, yn);
        const double w = xn[j] * step;
        sx[j] = sx[j] + w;
        if constexpr (QP) qx[j] = small_row_sum(a.Q, j, xn);      // Q x of the next iterate (x' is whole since the first barrier)
      }
      double *t0 = xs; xs = xn; xn = t0;
      double *t1 = ys; ys = yn; yn = t1;
      double *t2 = at; at = atn; atn = t2;
      wx = wx + step; wy = wy + step;
      __syncthreads();
    }
    trials = steps;
    if (tid == 0) { s_st[3] = wx; s_st[4] = wy; }
  }
  if constexpr (POLICY == SMALL_MALITSKY_POCK) {
    // take_step(::MalitskyPockStepsizeParameters) (pdhg.jl:555-647), an LP whose primal average is not empty (the
    // first-accept quirk, pdhg.jl:621-627, stays on the host)
    while (steps < a.n_steps && !num_err) {
      const double entry = s_st[1];
      const double tau = entry / a.primal_weight;
      // ---- K1 alone: x' = proj(x - tau (c - A'y)) with the step size on entry
      for (int j = tid; j < n; j += THREADS) {
        double v, b2;
        primal_one<false, false>(xs[j], cs[j], at[j], 0.0, lbs[j], ubs[j], tau, 0.0, v, b2);
        xn[j] = v;
      }
      if (tid == 0) s_st[0] = malitsky_pock_first_step(entry, s_st[2], a.interpolation_coefficient);
      __syncthreads();
      int acc_ok = 0;
      for (int it = 0; it < MALITSKY_POCK_MAX_TRIALS && !acc_ok; ++it) {
        const double step = s_st[0];
        const double ratio = step / entry, sigma = a.primal_weight * step;
        // ---- xbar = x' + ratio (x' - x)                                           (xbar_body, vector_kernels.hpp)
        for (int j = tid; j < n; j += THREADS) {
          const double v = xn[j];
          const double d = v - xs[j];
          const double t = ratio * d;
          xb[j] = v + t;
        }
        __syncthreads();
        // ---- K3 + K4: y' = proj(y + sigma (b - A xbar)), sum dy^2
        Acc3 acc = acc3_zero();
        for (int r = tid; r < m; r += THREADS) {
          const double s = small_row_sum(a.A, r, xb);
          const double yo = ys[r];
          const double dg = bs[r] - s;
          const double t = sigma * dg;
          double v = yo + t;
          if (r >= a.num_eq) v = jl_max(v, 0.0);
          yn[r] = v;
          const double dy = v - yo;
          dd_add(acc.hi[0], acc.lo[0], dy * dy);
        }
        __syncthreads();
        // ---- K5 + K6: A'y' and sum (A'y' - A'y)^2; both sums in one block reduction
        for (int j = tid; j < n; j += THREADS) {
          const double s = small_row_sum(a.T, j, yn);
          atn[j] = s;
          const double dd = s - at[j];
          dd_add(acc.hi[1], acc.lo[1], dd * dd);
        }
        block_sum_dd<2, THREADS>(acc, red);
        if (tid == 0) {
          double raw[5] = {0.0, 0.0, acc.hi[0] + acc.lo[0], acc.hi[1] + acc.lo[1], 0.0};
          const MalitskyPockRule rule = malitsky_pock_rule(raw, step, a.breaking_factor, a.downscaling_factor);
          s_dec[0] = (double)rule.accept;
          if (rule.accept) { s_st[1] = step; s_st[2] = ratio; s_st[3] = s_st[3] + entry; s_st[4] = s_st[4] + entry; }
          else s_st[0] = rule.next_step;
        }
        __syncthreads();
        acc_ok = __builtin_amdgcn_readfirstlane((int)(s_dec[0] != 0.0));
        trials += 1;
      }
      if (acc_ok) {
        // update_solution_in_solver_state (pdhg.jl:496-525) with the step size on entry as weight
        double *t0 = xs; xs = xn; xn = t0;
        double *t1 = ys; ys = yn; yn = t1;
        double *t2 = at; at = atn; atn = t2;
        for (int j = tid; j < n; j += THREADS) { const double t = xs[j] * entry; sx[j] = sx[j] + t; }
        for (int r = tid; r < m; r += THREADS) { const double t = ys[r] * entry; sy[r] = sy[r] + t; }
        steps += 1;
      } else num_err = 1;       // 60 rejections: x, y, the step size and the ratio stay as they came
      __syncthreads();
    }
  }
  for (int j = tid; j < n; j += THREADS) { a.x[j] = xs[j]; a.aty[j] = at[j]; a.sum_x[j] = sx[j]; }
  for (int r = tid; r < m; r += THREADS) { a.y[r] = ys[r]; a.sum_y[r] = sy[r]; }
  __syncthreads();
  if (tid == 0) {
    __threadfence_system();                // (the vectors written back above, not the result words)
    // steps_kernel's words (trial_kernel.hpp); [12]: ended inside a take_step (table exhausted), its step size on entry.
    // Malitsky-Pock: [0] the step size of the next take_step, [3] the ratio (neither moves in a take_step that failed)
    const double r[STEPS_RES_K] = {POLICY == SMALL_MALITSKY_POCK ? s_st[1] : s_st[0], (double)steps, (double)trials,
                                   POLICY == SMALL_MALITSKY_POCK ? s_st[2] : 0.0, 0.0, 0.0, s_st[3], s_st[4], (double)num_err, 0.0, 0.0, 0.0,
                                   mid ? s_st[1] : 0.0};
    publish_words(a.res_host, STEPS_RES_CAP, STEPS_RES_K, a.seq, [&](int q) { return r[q]; });
  }
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void small_lp_steps_kernel(SmallLpArgs a) {
  small_lp_steps_body<THREADS>(a);
}

// MANY small LPs in one launch (host_fleet.hpp): workgroup b runs entry b of `table` to the end of ITS n_steps, exactly
// as a solo launch would -- its own accepts and rejections, its own tables of powers (pointers into the call's shared
// pair), its own pinned result words.  The workgroups share nothing, so up to one per compute unit they run side by side;
// beyond that the dispatcher hands out the rest as compute units fall free (the table is ordered longest first).  The
// dynamic LDS of the launch is the largest member's; a smaller member uses the front of it.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void small_lp_fleet_kernel(const SmallLpArgs *__restrict__ table, int count) {
  if ((int)blockIdx.x >= count) return;
  const SmallLpArgs a = table[blockIdx.x];          // (uniform, read before any store: scalar loads)
  small_lp_steps_body<THREADS>(a);
}

// The two other policies: the same body behind kernels of their own names (the adaptive instantiations above keep theirs).
template <int THREADS>
__global__ __launch_bounds__(THREADS) void small_lp_constant_kernel(SmallLpArgs a) {
  small_lp_steps_body<THREADS, SMALL_CONSTANT>(a);
}
template <int THREADS>
__global__ __launch_bounds__(THREADS) void small_lp_malitsky_pock_kernel(SmallLpArgs a) {
  small_lp_steps_body<THREADS, SMALL_MALITSKY_POCK>(a);
}
template <int THREADS>
__global__ __launch_bounds__(THREADS) void small_fleet_constant_kernel(const SmallLpArgs *__restrict__ table, int count) {
  if ((int)blockIdx.x >= count) return;
  const SmallLpArgs a = table[blockIdx.x];
  small_lp_steps_body<THREADS, SMALL_CONSTANT>(a);
}
template <int THREADS>
__global__ __launch_bounds__(THREADS) void small_fleet_malitsky_pock_kernel(const SmallLpArgs *__restrict__ table, int count) {
  if ((int)blockIdx.x >= count) return;
  const SmallLpArgs a = table[blockIdx.x];
  small_lp_steps_body<THREADS, SMALL_MALITSKY_POCK>(a);
}

// The QP form (PDHG_SMALL_QP=1): the same body behind kernels of their own names, solo and fleet, for the adaptive and
// the constant policy.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void small_qp_steps_kernel(SmallQpArgs a) {
  small_lp_steps_body<THREADS, SMALL_ADAPTIVE, true>(a);
}
template <int THREADS>
__global__ __launch_bounds__(THREADS) void small_qp_fleet_kernel(const SmallQpArgs *__restrict__ table, int count) {
  if ((int)blockIdx.x >= count) return;
  const SmallQpArgs a = table[blockIdx.x];
  small_lp_steps_body<THREADS, SMALL_ADAPTIVE, true>(a);
}
template <int THREADS>
__global__ __launch_bounds__(THREADS) void small_qp_constant_kernel(SmallQpArgs a) {
  small_lp_steps_body<THREADS, SMALL_CONSTANT, true>(a);
}
template <int THREADS>
__global__ __launch_bounds__(THREADS) void small_qp_fleet_constant_kernel(const SmallQpArgs *__restrict__ table, int count) {
  if ((int)blockIdx.x >= count) return;
  const SmallQpArgs a = table[blockIdx.x];
  small_lp_steps_body<THREADS, SMALL_CONSTANT, true>(a);
}

}  // namespace
