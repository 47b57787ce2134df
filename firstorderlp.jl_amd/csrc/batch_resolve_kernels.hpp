// batch_resolve_kernels.hpp -- part of the single translation unit pdhg_hip.hip (included there, after resolve_kernels.hpp).
// RE-SOLVES of a BATCH on its handle (abi_batch_resolve.hpp, include/pdhg_hip_batch_resolve.h).  The members of a batch
// share the matrix, so they share the rescaling: ONE record of the applied steps (resolve_kernels.hpp: step-major,
// step s = its n column factors, then its m row factors) and one pair of running products serve all K members.
//
// The record is the dominant stream of a replay -- 8 S (n + m) bytes against 8 * 4 (n + m) per member -- so the replay
// reads it once per TILE of members instead of once per member: a thread owns element j and BATCH_RESOLVE_TILE members,
// walks the S steps once, loads each step's factor once and applies it to every member of its tile.  Consecutive lanes
// take consecutive j: every load and store of a wave is 64 consecutive doubles.  The arithmetic is
// resolve_replay_col / _row's, one rounding per step and quantity (c / d, lb * d, ub * d, b / e: plain operators, the
// build's -ffp-contract=off): the bits of a fresh pdhg_rescale of the same vectors.
//
// The tile is 4 members wide, chosen by the compiler's resource report for gfx950 (profiles/batch_resolve_throughput.txt).
// A column element keeps three live values per member and the fp64 divisions are expanded in line per member; the
// tile's 32 pointers are wave-uniform.  Width 2: 42 VGPRs, 8 waves per SIMD, nothing spilled; width 4: 77 VGPRs, 6 waves,
// 42 scalar registers parked in VGPR lanes (pointers, outside the loop over the steps); width 8: 111 VGPRs, 4 waves, 156
// parked.  No width uses scratch.  4 reads the record half as often as 2 and keeps six waves to cover its latency.
//
// Both kernels are grid-stride over max(n, m) with ew_grid's bounds in x; y is the member tile (replay) or the carried
// member (point).  Tables of the carried members lie in device memory, uploaded with the vectors in one copy.
#pragma once

namespace {

constexpr int BATCH_RESOLVE_TILE = 4;
static_assert(BATCH_MAX % BATCH_RESOLVE_TILE == 0, "the replay's member table is padded to whole tiles inside BATCH_MAX entries");

// table: one ResolveReplayMember per carried member; an entry that pads the last tile is all nullptr
__global__ __launch_bounds__(TPB) void batch_resolve_replay_kernel(int n, int m, int steps, const double *__restrict__ rec,
                                                                   const ResolveReplayMember *__restrict__ table) {
  constexpr int T = BATCH_RESOLVE_TILE;
  const int tid = blockIdx.x * TPB + threadIdx.x, st = gridDim.x * TPB;
  const int64_t stride = (int64_t)n + m;
  ResolveReplayMember M[T];
  bool cols = false, rows = false;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    M[t] = table[(size_t)blockIdx.y * T + t];
    cols = cols || M[t].in_c || M[t].in_lb || M[t].in_ub;
    rows = rows || M[t].in_b;
  }
  if (cols)
    for (int j = tid; j < n; j += st) {
      double vc[T], vl[T], vu[T];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        vc[t] = M[t].in_c ? M[t].in_c[j] : 0.0;
        vl[t] = M[t].in_lb ? M[t].in_lb[j] : 0.0;
        vu[t] = M[t].in_ub ? M[t].in_ub[j] : 0.0;
      }
      const double *f = rec + j;
      for (int s = 0; s < steps; ++s, f += stride) {
        const double d = *f;
#pragma unroll
        for (int t = 0; t < T; ++t) { vc[t] = vc[t] / d; vu[t] = vu[t] * d; vl[t] = vl[t] * d; }
      }
#pragma unroll
      for (int t = 0; t < T; ++t) {
        if (M[t].in_c) M[t].c[j] = vc[t];
        if (M[t].in_lb) M[t].lb[j] = vl[t];
        if (M[t].in_ub) M[t].ub[j] = vu[t];
      }
    }
  if (rows)
    for (int i = tid; i < m; i += st) {
      double vb[T];
#pragma unroll
      for (int t = 0; t < T; ++t) vb[t] = M[t].in_b ? M[t].in_b[i] : 0.0;
      const double *f = rec + n + i;
      for (int s = 0; s < steps; ++s, f += stride) {
        const double e = *f;
#pragma unroll
        for (int t = 0; t < T; ++t) vb[t] = vb[t] / e;
      }
#pragma unroll
      for (int t = 0; t < T; ++t) if (M[t].in_b) M[t].b[i] = vb[t];
    }
}

// One carried member of a warm start (resolve_point_col / _row's P, resolve_kernels.hpp).  pack_k >= 0: the scaled y also
// goes to Y[i * Kp + pack_k], where the batched product A' Y gathers it (batch_spmv_kernel<MODE_PLAIN>, batch_kernels.hpp).
struct BatchPointMember {
  const double *in_x, *in_y;
  double *x, *y, *aty;
  ResolveZeros z;
  int zero_aty, pack_k;
};

// cum_d / cum_e == nullptr (nothing was rescaled): the point is copied
__global__ __launch_bounds__(TPB) void batch_resolve_point_kernel(int n, int m, const double *__restrict__ cum_d,
                                                                  const double *__restrict__ cum_e,
                                                                  const BatchPointMember *__restrict__ table,
                                                                  double *__restrict__ Y, int shift) {
  const BatchPointMember a = table[blockIdx.y];
  const int tid = blockIdx.x * TPB + threadIdx.x, st = gridDim.x * TPB;
  for (int j = tid; j < n; j += st) resolve_point_col(a, cum_d, j);
  for (int i = tid; i < m; i += st) resolve_point_row(a, cum_e, i, Y, shift, a.pack_k);
}

// The front of a batch's staging buffers (pinned and device): the table of one call's carried members -- replay or
// point entries -- and, behind it, where the members' A'y are, by member slot (the batched product's output table).
constexpr size_t BATCH_RESOLVE_TABLE_BYTES = sizeof(BatchPointMember) * BATCH_MAX;
constexpr size_t BATCH_RESOLVE_HEAD_BYTES = BATCH_RESOLVE_TABLE_BYTES + sizeof(double *) * BATCH_MAX;
static_assert(sizeof(ResolveReplayMember) <= sizeof(BatchPointMember), "the replay table fits where the point table does");
static_assert(BATCH_RESOLVE_HEAD_BYTES % sizeof(double) == 0, "the vectors behind the head are aligned");

}  // namespace
