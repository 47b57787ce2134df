// vector_kernels.hpp -- part of the single translation unit pdhg_hip.hip (included there, in order).
// Elementwise PDHG kernels (primal step, xbar, interaction, accept/average) and the final reductions.
#pragma once

namespace {

// ---------------------------------------------------------------- elementwise

// K1+K2: x' = proj(x - tau*(Qx + c - A'y)), xbar = x' + theta*(x' - x).
//   compute_primal_gradient_from_dual_product  saddle_point.jl:1093-1100
//   next_primal = x .- (step/pw) .* g          pdhg.jl:466-467
//   projection!                                saddle_point.jl:87-92
//   xbar                                       pdhg.jl:486-487
template <bool HAS_Q, bool WRITE_XBAR>
__device__ __forceinline__ void primal_one(double x, double c, double aty,
                                           double qx, double lb, double ub,
                                           double tau, double theta, double &xn,
                                           double &xb) {
  const double q = HAS_Q ? qx : 0.0;
  const double t0 = q + c;
  const double g = t0 - aty;
  const double t1 = tau * g;
  double v = x - t1;
  v = jl_min(ub, jl_max(lb, v));
  xn = v;
  if (WRITE_XBAR) {
    const double d = v - x;
    const double t2 = theta * d;
    xb = v + t2;
  }
}

// A bound vector as primal_body reads it.  The dense array stays the authority (evaluation, getters, rescaling and
// the persistent kernels read it); the compact forms are DERIVED from it whenever it is written (bounds_rebuild,
// pdhg_hip.hip) and carry the same bit patterns, so the clamp sees exactly the operand a dense read gives it:
//   DENSE   the array itself;
//   CONST   every entry has the bit pattern of `def`: nothing is read;
//   SPARSE  `def` plus exceptions -- one mask bit per column, the number of exceptions before every block of
//           BND_BLOCK columns, and the exceptions' values packed in column order.  A block is what one wave covers
//           per grid-stride iteration below (64 pairs), so a wave reads ONE 16-byte mask entry and one count, and
//           a lane whose bit is set takes exc[blk[block] + (mask bits below its own)].
// Bounds of LPs are overwhelmingly 0 / +-inf (the benchmark LP: lb = 0, ub = +inf in 80 % of the columns), and
// rescaling leaves exactly those values as they are: 16 of primal_kernel's 72 B per column were spent on them.
enum { BND_DENSE = 0, BND_CONST = 1, BND_SPARSE = 2 };
constexpr int BND_BLOCK = 2 * WAVE;
struct BoundView {
  const double *dense;
  const unsigned long long *mask;   // [2 * blocks]: bit (j & 63) of word (j >> 6) set = column j is an exception
  const int *blk;                   // [blocks]: exceptions in the blocks before this one
  const double *exc;                // [exceptions]
  double def;
  int mode;
};
__host__ __device__ inline BoundView bound_dense(const double *p) { return BoundView{p, nullptr, nullptr, nullptr, 0.0, BND_DENSE}; }

// The streaming loads of the plain-launch primal_kernel (its `stream` argument, launch-uniform): every operand is read
// once per launch, and what the caches hold when the kernel ends should be the xbar it wrote, which the sweep behind it
// gathers from.  The builtin wants native vector types for the 16-byte loads.
typedef double nt_dbl2_t __attribute__((ext_vector_type(2)));
typedef unsigned long long nt_ull2_t __attribute__((ext_vector_type(2)));
// NT: the non-temporal form (known at compile time: a run-time choice between two loads of one address is folded into
// one load by the compiler, and the policy is lost)
template <bool NT>
__device__ __forceinline__ double2 ld_pair(const double *a, int p) {
  if (NT) {
    const nt_dbl2_t v = __builtin_nontemporal_load(reinterpret_cast<const nt_dbl2_t *>(a) + p);
    return double2{v.x, v.y};
  }
  return reinterpret_cast<const double2 *>(a)[p];
}

// entries 2p and 2p + 1
template <int BM, bool NT = false>
__device__ __forceinline__ double2 bound_pair(const BoundView &b, int p) {
  if (BM == BND_DENSE) return ld_pair<NT>(b.dense, p);
  double2 r = {b.def, b.def};
  if (BM == BND_SPARSE) {
    const int blk = p >> 6, l = p & 63;                 // one block per wave: both loads are one line per wave
    ulonglong2 w;
    int base;
    if (NT) {
      const nt_ull2_t t = __builtin_nontemporal_load(reinterpret_cast<const nt_ull2_t *>(b.mask) + blk);
      w.x = t.x; w.y = t.y;
      base = __builtin_nontemporal_load(b.blk + blk);
    } else {
      w = reinterpret_cast<const ulonglong2 *>(b.mask)[blk];
      base = b.blk[blk];
    }
    const unsigned long long mine = l < 32 ? w.x : w.y;
    const int sh = 2 * (l & 31);
    const unsigned bits = (unsigned)(mine >> sh) & 3u;
    if (bits) {
      const int rank = __popcll(mine & ((1ull << sh) - 1ull)) + (l < 32 ? 0 : __popcll(w.x));
      const double *e = b.exc + base + rank;
      if (NT) {
        if (bits & 1u) r.x = __builtin_nontemporal_load(e);
        if (bits & 2u) r.y = __builtin_nontemporal_load(e + (bits & 1u));
      } else {
        if (bits & 1u) r.x = e[0];
        if (bits & 2u) r.y = e[bits & 1u];
      }
    }
  }
  return r;
}
// entry j on its own (the odd tail), whatever the mode
__device__ __forceinline__ double bound_at(const BoundView &b, int j) {
  if (b.mode == BND_DENSE) return b.dense[j];
  if (b.mode == BND_SPARSE) {
    const int wd = j >> 6, bit = j & 63;
    const unsigned long long w = b.mask[wd];
    if ((w >> bit) & 1ull) {
      const int rank = __popcll(w & ((1ull << bit) - 1ull)) + ((wd & 1) ? __popcll(b.mask[wd - 1]) : 0);
      return b.exc[b.blk[j / BND_BLOCK] + rank];
    }
  }
  return b.def;
}

// Workgroup `bid` of `nb` (grid-stride; elementwise, so the distribution does not matter for the bits).
// COH: A'y -- and, for a QP, Q x -- was written by other compute units since this one last read it (multi-step trial
// kernel): coherent loads
// LBM / UBM: the modes of lb / ub, known at compile time (primal_kernel dispatches on them once per launch; shard
// slices and the persistent kernels pass DENSE views: the loads they always had)
// STREAM: non-temporal loads (the plain-launch primal_kernel alone asks for them; the pairs, not the odd tail)
template <bool HAS_Q, bool WRITE_XBAR, bool COH = false, int LBM = BND_DENSE, int UBM = BND_DENSE, bool STREAM = false>
__device__ __forceinline__ void primal_body(
    int n, const double *x, const double *c, const double *aty, const double *qx,
    const BoundView &lb, const BoundView &ub, double tau, double theta, double *x_next, double *xbar,
    double avg_w, double *sum_x, int bid, int nb, double avg_w2 = 0.0, double *sum_x_out = nullptr) {
  // sum_x != nullptr: the accept of the previous iteration left its K7 to this kernel
  // (sum_x += avg_w * x, x being the iterate accepted then; same two roundings)
  // sum_x_out != nullptr (only with sum_x): the paired form -- sum_x is read, not written, and
  // sum_x_out = (sum_x + avg_w * x) + avg_w2 * x' holds what the sums are once THIS trial is accepted with weight avg_w2
  // (the same additions in the same order as two single updates: pdhg_accept then swaps the buffers)
  const int npair = n >> 1;
  const int stride = nb * TPB;
  for (int p = bid * TPB + threadIdx.x; p < npair; p += stride) {
    const double2 xv = ld_pair<STREAM>(x, p);
    double2 sv = {0.0, 0.0};
    if (sum_x) {
      sv = ld_pair<STREAM>(sum_x, p);
      const double t0 = xv.x * avg_w, t1 = xv.y * avg_w;
      sv.x = sv.x + t0;
      sv.y = sv.y + t1;
      if (!sum_x_out) reinterpret_cast<double2 *>(sum_x)[p] = sv;
    }
    const double2 cv = ld_pair<STREAM>(c, p);
    double2 av;
    if (COH) { av.x = ldc<true>(aty + 2 * p); av.y = ldc<true>(aty + 2 * p + 1); }
    else av = ld_pair<STREAM>(aty, p);
    const double2 lv = bound_pair<LBM, STREAM>(lb, p);
    const double2 uv = bound_pair<UBM, STREAM>(ub, p);
    double2 qv = {0.0, 0.0};
    if (HAS_Q) {
      if (COH) { qv.x = ldc<true>(qx + 2 * p); qv.y = ldc<true>(qx + 2 * p + 1); }
      else qv = ld_pair<STREAM>(qx, p);
    }
    double2 xn, xb;
    primal_one<HAS_Q, WRITE_XBAR>(xv.x, cv.x, av.x, qv.x, lv.x, uv.x, tau, theta, xn.x, xb.x);
    primal_one<HAS_Q, WRITE_XBAR>(xv.y, cv.y, av.y, qv.y, lv.y, uv.y, tau, theta, xn.y, xb.y);
    {
      reinterpret_cast<double2 *>(x_next)[p] = xn;
      if (WRITE_XBAR) reinterpret_cast<double2 *>(xbar)[p] = xb;
    }
    if (sum_x_out) {
      const double u0 = xn.x * avg_w2, u1 = xn.y * avg_w2;
      sv.x = sv.x + u0;
      sv.y = sv.y + u1;
      reinterpret_cast<double2 *>(sum_x_out)[p] = sv;
    }
  }
  if ((n & 1) && bid == 0 && threadIdx.x == 0) {
    const int j = n - 1;
    double xn, xb;
    double sv = 0.0;
    if (sum_x) {
      const double t = x[j] * avg_w;
      sv = sum_x[j] + t;
      if (!sum_x_out) sum_x[j] = sv;
    }
    primal_one<HAS_Q, WRITE_XBAR>(x[j], c[j], ldc<COH>(aty + j), HAS_Q ? ldc<COH>(qx + j) : 0.0, bound_at(lb, j), bound_at(ub, j), tau, theta, xn, xb);
    x_next[j] = xn;
    if (WRITE_XBAR) xbar[j] = xb;
    if (sum_x_out) {
      const double u = xn * avg_w2;
      sum_x_out[j] = sv + u;
    }
  }
}

template <bool HAS_Q, bool WRITE_XBAR>
__global__ __launch_bounds__(TPB) void primal_kernel(
    int n, const double *__restrict__ x, const double *__restrict__ c,
    const double *__restrict__ aty, const double *__restrict__ qx,
    BoundView lb, BoundView ub, double tau,
    double theta, double *__restrict__ x_next, double *__restrict__ xbar,
    double avg_w, double *__restrict__ sum_x, double avg_w2, double *__restrict__ sum_x_out, int stream) {
#define PDHG_PB_S(L, U, S)                                                                                              \
  primal_body<HAS_Q, WRITE_XBAR, false, L, U, S>(n, x, c, aty, qx, lb, ub, tau, theta, x_next, xbar, avg_w, sum_x, blockIdx.x, gridDim.x, \
                                                 avg_w2, sum_x_out)
#define PDHG_PB(L, U)                                                                                                   \
  do {                                                                                                                  \
    if (stream) PDHG_PB_S(L, U, true);                                                                                  \
    else PDHG_PB_S(L, U, false);                                                                                        \
  } while (0)
  switch (lb.mode * 3 + ub.mode) {        // launch-uniform: one loop per pair of modes, no test inside it
    case BND_DENSE * 3 + BND_CONST: PDHG_PB(BND_DENSE, BND_CONST); break;
    case BND_DENSE * 3 + BND_SPARSE: PDHG_PB(BND_DENSE, BND_SPARSE); break;
    case BND_CONST * 3 + BND_DENSE: PDHG_PB(BND_CONST, BND_DENSE); break;
    case BND_CONST * 3 + BND_CONST: PDHG_PB(BND_CONST, BND_CONST); break;
    case BND_CONST * 3 + BND_SPARSE: PDHG_PB(BND_CONST, BND_SPARSE); break;
    case BND_SPARSE * 3 + BND_DENSE: PDHG_PB(BND_SPARSE, BND_DENSE); break;
    case BND_SPARSE * 3 + BND_CONST: PDHG_PB(BND_SPARSE, BND_CONST); break;
    case BND_SPARSE * 3 + BND_SPARSE: PDHG_PB(BND_SPARSE, BND_SPARSE); break;
    default: PDHG_PB(BND_DENSE, BND_DENSE); break;
  }
#undef PDHG_PB
#undef PDHG_PB_S
}

// ---- building the compact forms (bounds_rebuild, pdhg_hip.hip) ----
// Bit patterns, not values: -0.0 and +0.0 are different defaults, and a NaN equals itself.
// cnt[q] = entries with the bits of candidate q: the first entry's, +inf, -inf, +0.0
__global__ __launch_bounds__(TPB) void bound_census_kernel(int n, const double *__restrict__ v, unsigned *__restrict__ cnt) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int gw = (blockIdx.x * TPB + threadIdx.x) / WAVE, nw = gridDim.x * (TPB / WAVE);
  const unsigned long long cand[4] = {(unsigned long long)__double_as_longlong(v[0]), 0x7FF0000000000000ull,
                                      0xFFF0000000000000ull, 0ull};
  unsigned c[4] = {0u, 0u, 0u, 0u};
  for (int64_t base = (int64_t)gw * WAVE; base < n; base += (int64_t)nw * WAVE) {      // wave-uniform
    const int64_t j = base + lane;
    const bool ok = j < n;
    const unsigned long long b = ok ? (unsigned long long)__double_as_longlong(v[j]) : 0ull;
#pragma unroll
    for (int q = 0; q < 4; ++q) c[q] += (unsigned)__popcll(__ballot(ok && b == cand[q]));
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) if (c[q]) atomicAdd(cnt + q, c[q]);
  }
}
// one wave per block of BND_BLOCK columns: its two mask words and its number of exceptions
__global__ __launch_bounds__(TPB) void bound_mask_kernel(int n, const double *__restrict__ v, unsigned long long def,
                                                         unsigned long long *__restrict__ mask, int *__restrict__ cnt) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int gw = (blockIdx.x * TPB + threadIdx.x) / WAVE, nw = gridDim.x * (TPB / WAVE);
  const int nblk = (n + BND_BLOCK - 1) / BND_BLOCK;
  for (int b = gw; b < nblk; b += nw) {                                                // wave-uniform
    const int64_t j0 = (int64_t)b * BND_BLOCK + lane, j1 = j0 + WAVE;
    const unsigned long long w0 = __ballot(j0 < n && (unsigned long long)__double_as_longlong(v[j0 < n ? j0 : 0]) != def);
    const unsigned long long w1 = __ballot(j1 < n && (unsigned long long)__double_as_longlong(v[j1 < n ? j1 : 0]) != def);
    if (lane == 0) {
      mask[2 * (size_t)b] = w0;
      mask[2 * (size_t)b + 1] = w1;
      cnt[b] = __popcll(w0) + __popcll(w1);
    }
  }
}
// the exceptions' values, packed in column order behind their block's offset
__global__ __launch_bounds__(TPB) void bound_pack_kernel(int n, const double *__restrict__ v,
                                                         const unsigned long long *__restrict__ mask,
                                                         const int *__restrict__ blk, double *__restrict__ exc) {
  const int stride = gridDim.x * TPB;
  for (int j = blockIdx.x * TPB + threadIdx.x; j < n; j += stride) {
    const int wd = j >> 6, bit = j & 63;
    const unsigned long long w = mask[wd];
    if ((w >> bit) & 1ull) {
      const int rank = __popcll(w & ((1ull << bit) - 1ull)) + ((wd & 1) ? __popcll(mask[wd - 1]) : 0);
      exc[blk[j / BND_BLOCK] + rank] = v[j];
    }
  }
}

// xbar = x' + theta*(x' - x) on its own (Malitsky-Pock retries, pdhg.jl:590-601)
__device__ __forceinline__ void xbar_body(int n, const double *x, const double *x_next, double theta, double *xbar,
                                          int bid, int nb) {
  const int stride = nb * TPB;
  for (int j = bid * TPB + threadIdx.x; j < n; j += stride) {
    const double v = x_next[j];
    const double d = v - x[j];
    const double t = theta * d;
    xbar[j] = v + t;
  }
}
__global__ __launch_bounds__(TPB) void xbar_kernel(int n, const double *__restrict__ x,
                                                   const double *__restrict__ x_next,
                                                   double theta, double *__restrict__ xbar) {
  xbar_body(n, x, x_next, theta, xbar, blockIdx.x, gridDim.x);
}

// dx = x' - x  (for the QP interaction term 0.5*dx'Q dx, pdhg.jl:536-541)
__device__ __forceinline__ void diff_body(int n, const double *a, const double *b, double *out, int bid, int nb) {
  const int stride = nb * TPB;
  for (int j = bid * TPB + threadIdx.x; j < n; j += stride) out[j] = a[j] - b[j];
}
// the same with primal_body's element-to-thread mapping (pairs 2p, 2p + 1; the odd tail on block 0, thread 0):
// inside the one-launch trial kernel every thread then reads back only the x' it has just written itself
__device__ __forceinline__ void diff_pairs_body(int n, const double *a, const double *b, double *out, int bid, int nb) {
  const int npair = n >> 1;
  const int stride = nb * TPB;
  for (int p = bid * TPB + threadIdx.x; p < npair; p += stride) {
    out[2 * p] = a[2 * p] - b[2 * p];
    out[2 * p + 1] = a[2 * p + 1] - b[2 * p + 1];
  }
  if ((n & 1) && bid == 0 && threadIdx.x == 0) out[n - 1] = a[n - 1] - b[n - 1];
}
// xbar_body's expression with the same mapping: the multi-step Malitsky-Pock kernel forms xbar -- again after every
// rejected dual trial -- from the x' the thread wrote itself in the primal step
__device__ __forceinline__ void xbar_pairs_body(int n, const double *x, const double *x_next, double theta, double *xbar, int bid, int nb) {
  const int npair = n >> 1;
  const int stride = nb * TPB;
  auto one = [&](int j) {
    const double v = x_next[j];
    const double d = v - x[j];
    const double t = theta * d;
    xbar[j] = v + t;
  };
  for (int p = bid * TPB + threadIdx.x; p < npair; p += stride) { one(2 * p); one(2 * p + 1); }
  if ((n & 1) && bid == 0 && threadIdx.x == 0) one(n - 1);
}
__global__ __launch_bounds__(TPB) void diff_kernel(int n, const double *__restrict__ a,
                                                   const double *__restrict__ b,
                                                   double *__restrict__ out) {
  diff_body(n, a, b, out, blockIdx.x, gridDim.x);
}

// Reductions over the replicated n-vectors (row-partitioned form, after the
// all-reduce delivered A'y'):  dx.(A'y'-A'y), dx^2, (A'y'-A'y)^2.
__global__ __launch_bounds__(TPB) void interaction_kernel(
    int n, const double *__restrict__ x, const double *__restrict__ x_next,
    const double *__restrict__ aty, const double *__restrict__ aty_next,
    double *__restrict__ partials, int pstride) {
  __shared__ double red[6][TPB / WAVE];
  Acc3 acc = acc3_zero();
  const int stride = gridDim.x * TPB;
  for (int j = blockIdx.x * TPB + threadIdx.x; j < n; j += stride) {
    const double dx = x_next[j] - x[j];
    const double dd = aty_next[j] - aty[j];
    dd_add(acc.hi[0], acc.lo[0], dx * dd);
    dd_add(acc.hi[1], acc.lo[1], dx * dx);
    dd_add(acc.hi[2], acc.lo[2], dd * dd);
  }
  block_sum_dd<3, TPB>(acc, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      partials[q * pstride + blockIdx.x] = acc.hi[q];
      partials[(3 + q) * pstride + blockIdx.x] = acc.lo[q];
    }
  }
}

// dot(a, b) partials (QP term), double-double: block `bid` of `nb` writes partials[bid] (hi) and partials[nb + bid] (lo)
// COH: a and b were rewritten by other compute units since this one last read them (multi-step trial kernel)
template <bool COH = false>
__device__ __forceinline__ void dot_body(int n, const double *a, const double *b, double *partials, int bid, int nb,
                                         double (*red)[TPB / WAVE], bool agent_store) {
  Acc3 acc = acc3_zero();
  const int stride = nb * TPB;
  for (int j = bid * TPB + threadIdx.x; j < n; j += stride) dd_add(acc.hi[0], acc.lo[0], ldc<COH>(a + j) * ldc<COH>(b + j));
  block_sum_dd<1, TPB>(acc, red);
  if (threadIdx.x == 0) {
    if (agent_store) {
      __hip_atomic_store(partials + bid, acc.hi[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(partials + nb + bid, acc.lo[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      partials[bid] = acc.hi[0];
      partials[nb + bid] = acc.lo[0];
    }
  }
}
__global__ __launch_bounds__(TPB) void dot_kernel(int n, const double *__restrict__ a,
                                                  const double *__restrict__ b,
                                                  double *__restrict__ partials) {
  __shared__ double red[6][TPB / WAVE];
  dot_body(n, a, b, partials, blockIdx.x, gridDim.x, red, false);
}

// K7: sum_x += w*x', sum_y += w*y'      saddle_point.jl:258-259, 271
__global__ __launch_bounds__(TPB) void accept_kernel(int n, int m, double w,
                                                     const double *__restrict__ xs,
                                                     double *__restrict__ sum_x,
                                                     const double *__restrict__ ys,
                                                     double *__restrict__ sum_y) {
  const int stride = gridDim.x * TPB;
  const int tid = blockIdx.x * TPB + threadIdx.x;
  for (int j = tid; j < n; j += stride) {
    const double t = xs[j] * w;
    sum_x[j] = sum_x[j] + t;
  }
  for (int i = tid; i < m; i += stride) {
    const double t = ys[i] * w;
    sum_y[i] = sum_y[i] + t;
  }
}

// compute_average: sum / weight (a division, saddle_point.jl:296-301)
__global__ __launch_bounds__(TPB) void div_kernel(int n, const double *__restrict__ s,
                                                  double w, double *__restrict__ out) {
  const int stride = gridDim.x * TPB;
  for (int j = blockIdx.x * TPB + threadIdx.x; j < n; j += stride) out[j] = s[j] / w;
}

// Second-stage, fixed-order sum of the block partials.  One workgroup.
// spec[q] = {ptr, count}; out[q] = sum(ptr[0..count)).  count==0 -> 0.
struct FinalSpec {
  const double *ptr[5];     // hi parts of the block partials
  const double *ptr_lo[5];  // lo parts
  int count[5];
  double *out;     // 5 doubles (host-mapped or device)
};
// The five sums, each a double-double sum of its block partials: quantity q is summed by three
// "virtual waves" 3q..3q+2 (strided per-lane sums, wave shuffle tree, then the three wave totals
// left to right -- a fixed order, although the double-double result does not depend on it except
// with negligible probability).  A workgroup of NW waves runs virtual wave v on wave v mod NW: the
// separate final kernels have 16 waves (one virtual wave each), the one-launch trial kernel 4 --
// the arithmetic, hence the bits, are the same.  Thread 0 ends with all five, rounded to one
// double each, in res[].
#ifndef PDHG_FINAL_BATCH
#define PDHG_FINAL_BATCH 4
#endif
template <int NW>
__device__ __forceinline__ void final_reduce_body(const FinalSpec &sp, double (&res)[5]) {
  __shared__ double wsum[16], wsum_lo[16];
  const int wid = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  constexpr int VPW = (15 + NW - 1) / NW;        // virtual waves per physical wave
  // load pairs in flight per lane and virtual wave (registers: 2 * VPW * B doubles).  The 4-wave form (trial kernel) takes 5:
  // a one-launch LP has up to ~1000 block partials per quantity, i.e. 5 per lane and virtual wave -- one trip to memory
  constexpr int B = NW >= 16 ? PDHG_FINAL_BATCH : PDHG_FINAL_BATCH + 1;
  // The partials come from other CUs' stores: every load is a trip to memory.  All of a
  // physical wave's first B loads per virtual wave are requested before anything is added
  // (one round trip instead of VPW).
  double th[VPW][B], tl[VPW][B];
#pragma unroll
  for (int j = 0; j < VPW; ++j) {
    const int v = wid + j * NW;
    const int q = v < 15 ? v / 3 : 0, sub = v % 3;
    const double *p = sp.ptr[q], *pl = sp.ptr_lo[q];
    const int cnt = v < 15 ? sp.count[q] : 0;
#pragma unroll
    for (int u = 0; u < B; ++u) {
      const int i = sub * WAVE + lane + u * 3 * WAVE;
      th[j][u] = i < cnt ? p[i] : 0.0;
      tl[j][u] = i < cnt ? pl[i] : 0.0;
    }
  }
#pragma unroll
  for (int j = 0; j < VPW; ++j) {
    const int v = wid + j * NW;
    if (v < 15) {                                 // wave-uniform
      const int q = v / 3, sub = v % 3;
      const double *p = sp.ptr[q], *pl = sp.ptr_lo[q];
      const int cnt = sp.count[q];
      double hi = 0.0, lo = 0.0;
#pragma unroll
      for (int u = 0; u < B; ++u)
        if (sub * WAVE + lane + u * 3 * WAVE < cnt) dd_add_dd(hi, lo, th[j][u], tl[j][u]);
      for (int i0 = sub * WAVE + lane + B * 3 * WAVE; i0 < cnt; i0 += B * 3 * WAVE) {
        double rh[B], rl[B];
#pragma unroll
        for (int u = 0; u < B; ++u) {
          const int i = i0 + u * 3 * WAVE;
          rh[u] = i < cnt ? p[i] : 0.0;
          rl[u] = i < cnt ? pl[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < B; ++u)
          if (i0 + u * 3 * WAVE < cnt) dd_add_dd(hi, lo, rh[u], rl[u]);
      }
      wave_sum_dd(hi, lo);
      if (lane == WAVE - 1) { wsum[v] = hi; wsum_lo[v] = lo; }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      double hi = wsum[3 * k], lo = wsum_lo[3 * k];
      dd_add_dd(hi, lo, wsum[3 * k + 1], wsum_lo[3 * k + 1]);
      dd_add_dd(hi, lo, wsum[3 * k + 2], wsum_lo[3 * k + 2]);
      res[k] = hi + lo;
    }
  }
}

// The same second stage for an LP (quantity 4, dx'Q dx, is absent) with ONE WAVE PER QUANTITY: wave q adds quantity q,
// B load pairs per lane in flight at a time -- a handful of registers (the general form above keeps 2 * 4 * 5 doubles
// in flight per lane and spills inside the multi-step kernel: 11.4 us from "barrier complete" to "decision known" on a
// 40-workgroup grid, 2.9 us with this one).  Exactly rounded double-double sums: the same bits whatever the grouping.
// Called by a 4-wave workgroup; lds8: 8 doubles of LDS.
__device__ __forceinline__ bool final_reduce_lp_ok(const FinalSpec &sp) { return sp.count[4] == 0; }
template <int B>
__device__ __forceinline__ void final_reduce_lp(const FinalSpec &sp, double (&res)[5], double *lds8) {
  const int wid = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const double *p = sp.ptr[wid], *pl = sp.ptr_lo[wid];
  const int cnt = sp.count[wid];
  double hi = 0.0, lo = 0.0;
  for (int base = 0; base < cnt; base += B * WAVE) {         // wave-uniform trip count
    double h[B], l[B];
#pragma unroll
    for (int u = 0; u < B; ++u) {
      const int i = base + lane + u * WAVE;
      h[u] = i < cnt ? p[i] : 0.0;
      l[u] = i < cnt ? pl[i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < B; ++u)
      if (base + lane + u * WAVE < cnt) dd_add_dd(hi, lo, h[u], l[u]);
  }
  wave_sum_dd(hi, lo);
  if (lane == WAVE - 1) { lds8[wid] = hi; lds8[4 + wid] = lo; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) res[k] = lds8[k] + lds8[4 + k];
    res[4] = 0.0;
  }
}

// The same for a QP: wave q adds quantity q as above, and the fifth quantity, dx . (Q'dx), is added the way
// final_reduce_body adds it -- waves 0, 1, 2 are its three virtual waves (strided per-lane sums in index order, the wave
// tree, the three totals left to right) -- so its bits are that function's by construction.  Its first B4 load pairs
// per lane (all of them up to B4 * 3 * WAVE partials, n <= 147 456) are requested in front of the wave's own quantity.
// lds14: 14 doubles of LDS.
template <int B, int B4>
__device__ __forceinline__ void final_reduce_qp(const FinalSpec &sp, double (&res)[5], double *lds14) {
  const int wid = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const double *p4 = sp.ptr[4], *pl4 = sp.ptr_lo[4];
  const int cnt4 = wid < 3 ? sp.count[4] : 0, i4 = wid * WAVE + lane;
  double h4[B4], l4[B4];
#pragma unroll
  for (int u = 0; u < B4; ++u) {
    const int i = i4 + u * 3 * WAVE;
    h4[u] = i < cnt4 ? p4[i] : 0.0;
    l4[u] = i < cnt4 ? pl4[i] : 0.0;
  }
  const double *p = sp.ptr[wid], *pl = sp.ptr_lo[wid];
  const int cnt = sp.count[wid];
  double hi = 0.0, lo = 0.0;
  for (int base = 0; base < cnt; base += B * WAVE) {         // wave-uniform trip count
    double h[B], l[B];
#pragma unroll
    for (int u = 0; u < B; ++u) {
      const int i = base + lane + u * WAVE;
      h[u] = i < cnt ? p[i] : 0.0;
      l[u] = i < cnt ? pl[i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < B; ++u)
      if (base + lane + u * WAVE < cnt) dd_add_dd(hi, lo, h[u], l[u]);
  }
  wave_sum_dd(hi, lo);
  if (lane == WAVE - 1) { lds14[wid] = hi; lds14[4 + wid] = lo; }
  if (wid < 3) {                                              // wave-uniform
    hi = 0.0; lo = 0.0;
#pragma unroll
    for (int u = 0; u < B4; ++u)
      if (i4 + u * 3 * WAVE < cnt4) dd_add_dd(hi, lo, h4[u], l4[u]);
    for (int i = i4 + B4 * 3 * WAVE; i < cnt4; i += 3 * WAVE) dd_add_dd(hi, lo, p4[i], pl4[i]);
    wave_sum_dd(hi, lo);
    if (lane == WAVE - 1) { lds14[8 + wid] = hi; lds14[11 + wid] = lo; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) res[k] = lds14[k] + lds14[4 + k];
    double h = lds14[8], l = lds14[11];
    dd_add_dd(h, l, lds14[9], lds14[12]);
    dd_add_dd(h, l, lds14[10], lds14[13]);
    res[4] = h + l;
  }
}

__global__ __launch_bounds__(FINAL_TPB) void final_reduce_kernel(FinalSpec sp) {
  double res[5];
  final_reduce_body<FINAL_TPB / WAVE>(sp, res);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) sp.out[k] = res[k];
  }
}

}  // namespace
