// resolve_kernels.hpp -- part of the single translation unit pdhg_hip.hip (included there, after batch_kernels.hpp).
// RE-SOLVES on a live handle (abi_resolve.hpp, include/pdhg_hip_resolve.h): new c / b / lb / ub in the space pdhg_create
// took them in, brought to the handle's working space by replaying the diagonal rescaling steps pdhg_rescale applied, and
// a starting point brought there by the cumulative factors.
//
// The record is STEP-MAJOR: step s occupies rec[s * (n + m) ...): its n column factors, then its m row factors -- the
// t.dv / t.ev of that apply_scaling step.  A thread owns one element and walks the steps; at every step a wave reads 64
// consecutive doubles of the record.  The arithmetic is resc_apply_vectors_kernel's, one rounding per step and quantity
// (c / d, lb * d, ub * d, b / e: plain operators, the build's -ffp-contract=off and the correctly rounded fp64 division
// are what makes the result the bits of a fresh pdhg_rescale of the same vectors).
//
// Streaming fp64 elementwise kernels: grid-stride over max(n, m) like the other elementwise kernels (ew_grid); the fleet
// forms take their work as (member, chunk of elements) items from a table in device memory, one workgroup per item
// (small_lp_fleet_kernel's pattern): a large member gets several workgroups, a 27 x 32 member one.
#pragma once

namespace {

// one retained apply_scaling step: its factors into the record, the running products beside resc_apply_vectors_kernel's
// (the same multiplications from 1.0 in the same order: the same bits as the arrays pdhg_rescale returns)
// (the element bodies, shared with fleet_rescale_kernel)
__device__ __forceinline__ void resolve_record_col(double d, double *rec_step, double *cum_d, int j) {
  rec_step[j] = d; cum_d[j] = cum_d[j] * d;
}
__device__ __forceinline__ void resolve_record_row(double e, double *rec_step, double *cum_e, int n, int i) {
  rec_step[(int64_t)n + i] = e; cum_e[i] = cum_e[i] * e;
}
__global__ __launch_bounds__(TPB) void resolve_record_kernel(int n, int m, const double *__restrict__ dv,
                                                             const double *__restrict__ ev, double *__restrict__ rec_step,
                                                             double *__restrict__ cum_d, double *__restrict__ cum_e) {
  const int tid = blockIdx.x * TPB + threadIdx.x, st = gridDim.x * TPB;
  for (int j = tid; j < n; j += st) resolve_record_col(dv[j], rec_step, cum_d, j);
  for (int i = tid; i < m; i += st) resolve_record_row(ev[i], rec_step, cum_e, n, i);
}

// One member of a replay.  in_* == nullptr: that vector keeps what it holds -- no load, no store.
struct ResolveReplayMember {
  const double *in_c, *in_lb, *in_ub, *in_b;      // create space (device staging)
  double *c, *lb, *ub, *b;                        // the member's working vectors
};
struct ResolveReplayArgs {
  int n, m, steps;
  const double *rec;                              // [steps][n + m]
  ResolveReplayMember v;
};

// What one element of a replay does.  (The batch's replay, batch_resolve_kernels.hpp, is this arithmetic over a tile of
// members; the two are not one template: instantiated at a tile of 1 it costs these kernels two more VGPRs than this
// form does, profiles/resolve_throughput.txt.)
__device__ __forceinline__ void resolve_replay_col(const ResolveReplayArgs &a, int j) {
  const int64_t stride = (int64_t)a.n + a.m;
  const ResolveReplayMember &v = a.v;
  double vc = v.in_c ? v.in_c[j] : 0.0, vl = v.in_lb ? v.in_lb[j] : 0.0, vu = v.in_ub ? v.in_ub[j] : 0.0;
  const double *f = a.rec + j;
  for (int s = 0; s < a.steps; ++s, f += stride) {
    const double d = *f;
    vc = vc / d; vu = vu * d; vl = vl * d;
  }
  if (v.in_c) v.c[j] = vc;
  if (v.in_lb) v.lb[j] = vl;
  if (v.in_ub) v.ub[j] = vu;
}
__device__ __forceinline__ void resolve_replay_row(const ResolveReplayArgs &a, int i) {
  const int64_t stride = (int64_t)a.n + a.m;
  double vb = a.v.in_b[i];
  const double *f = a.rec + a.n + i;
  for (int s = 0; s < a.steps; ++s, f += stride) vb = vb / *f;
  a.v.b[i] = vb;
}

__global__ __launch_bounds__(TPB) void resolve_replay_kernel(ResolveReplayArgs a) {
  const int tid = blockIdx.x * TPB + threadIdx.x, st = gridDim.x * TPB;
  if (a.v.in_c || a.v.in_lb || a.v.in_ub)
    for (int j = tid; j < a.n; j += st) resolve_replay_col(a, j);
  if (a.v.in_b)
    for (int i = tid; i < a.m; i += st) resolve_replay_row(a, i);
}

// A starting point in create space to the working space: x_s = x * cum_d, y_s = y * cum_e (the output divides by these,
// preprocess.jl); cum_* == nullptr (nothing was rescaled): a copy.  in_x / in_y == nullptr: zeros.  zero_aty: A'y of
// y = 0 as a fresh handle holds it, +0.0 (the product itself could leave -0.0 in a column of negative entries).
// ResolveZeros: the n- / m-vectors a fresh handle holds zeros in (resolve_fresh_zeros, host_resolve.hpp, names them),
// zeroed in the same pass; nullptr: not allocated yet.
struct ResolveZeros {
  double *zn[5], *zm[3];
};
struct ResolvePointArgs {
  int n, m, zero_aty;
  const double *in_x, *in_y, *cum_d, *cum_e;
  double *x, *y, *aty;
  ResolveZeros z;
};

// What one element of a warm start does; P: ResolvePointArgs, or a batch's BatchPointMember (the running products are the
// batch's).  pack_k >= 0: the scaled y also goes to Y[(i << shift) + pack_k] (a batch's interleaved Y).
template <class P>
__device__ __forceinline__ void resolve_point_col(const P &a, const double *cum_d, int j) {
  double v = 0.0;
  if (a.in_x) { v = a.in_x[j]; if (cum_d) v = v * cum_d[j]; }
  a.x[j] = v;
  if (a.zero_aty) a.aty[j] = 0.0;
#pragma unroll
  for (int q = 0; q < 5; ++q) if (a.z.zn[q]) a.z.zn[q][j] = 0.0;
}
template <class P>
__device__ __forceinline__ void resolve_point_row(const P &a, const double *cum_e, int i, double *Y = nullptr, int shift = 0, int pack_k = -1) {
  double v = 0.0;
  if (a.in_y) { v = a.in_y[i]; if (cum_e) v = v * cum_e[i]; }
  a.y[i] = v;
  if (pack_k >= 0) Y[((size_t)i << shift) + pack_k] = v;
#pragma unroll
  for (int q = 0; q < 3; ++q) if (a.z.zm[q]) a.z.zm[q][i] = 0.0;
}

__global__ __launch_bounds__(TPB) void resolve_point_kernel(ResolvePointArgs a) {
  const int tid = blockIdx.x * TPB + threadIdx.x, st = gridDim.x * TPB;
  for (int j = tid; j < a.n; j += st) resolve_point_col(a, a.cum_d, j);
  for (int i = tid; i < a.m; i += st) resolve_point_row(a, a.cum_e, i);
}

// ---- the fleet forms: one workgroup per (member, chunk) item; elements [lo, hi) of the member's max(n, m) ----
constexpr int RESOLVE_CHUNK = 4 * TPB;

struct FleetResolveReplayItem {
  ResolveReplayArgs a;
  int lo, hi;
};
struct FleetResolvePointItem {
  ResolvePointArgs a;
  int lo, hi;
};

__global__ __launch_bounds__(TPB) void fleet_resolve_replay_kernel(const FleetResolveReplayItem *__restrict__ table, int count) {
  if ((int)blockIdx.x >= count) return;
  const FleetResolveReplayItem it = table[blockIdx.x];
  const ResolveReplayArgs &a = it.a;
  if (a.v.in_c || a.v.in_lb || a.v.in_ub)
    for (int j = it.lo + threadIdx.x; j < min(it.hi, a.n); j += TPB) resolve_replay_col(a, j);
  if (a.v.in_b)
    for (int i = it.lo + threadIdx.x; i < min(it.hi, a.m); i += TPB) resolve_replay_row(a, i);
}

__global__ __launch_bounds__(TPB) void fleet_resolve_point_kernel(const FleetResolvePointItem *__restrict__ table, int count) {
  if ((int)blockIdx.x >= count) return;
  const FleetResolvePointItem it = table[blockIdx.x];
  const ResolvePointArgs &a = it.a;
  for (int j = it.lo + threadIdx.x; j < min(it.hi, a.n); j += TPB) resolve_point_col(a, a.cum_d, j);
  for (int i = it.lo + threadIdx.x; i < min(it.hi, a.m); i += TPB) resolve_point_row(a, a.cum_e, i);
}

}  // namespace
