// matrix_update_kernels.hpp -- part of the single translation unit pdhg_hip.hip (included there, after the other kernel headers).
// NEW MATRIX VALUES on a kept sparsity pattern (include/pdhg_hip_matrix_update.h; host side in abi_matrix_update.hpp).
//
// CSR(A') is the caller's CSC narrowed to 32 bits, so its values are the caller's array as it is.  Every
// other resident copy holds the same entries in another order.  The kernels below walk a copy exactly as the scale
// kernels of rescale_kernels.hpp do -- the same decode of (row, column) for every stored slot -- and STORE the entry's
// value, looked up by a binary search, where those multiply:
//   CSR(A)                     slot (i, j): row j of CSR(A'), searched for i          (TRANSPOSED = true)
//   column slabs, sweep copy   slot (i, j): row i of the matrix's own CSR, for j      (TRANSPOSED = false)
// The search needs the searched run to ascend strictly: true of every row of CSR(A) by construction (the builders visit
// the columns in order), and of CSR(A') when the caller's columns hold ascending row indices without duplicates
// (mu_ascending_kernel; a handle that was created from other columns is refused).  Nothing is kept between calls: no
// permutation, no per-nonzero array.
//
// All kernels are templates, so that their instances lie in the code object where abi_matrix_update.hpp first names
// them -- behind everything that was there before (pdhg_hip.hip, "Code placement").
#pragma once

namespace {

// one piece of a searched matrix: a CsrDev without segments, or one row segment (rows [row0, row0 + rows))
struct MuPiece {
  int row0, rows;
  const int *rowptr, *col;
  const double *val;
};
// the searched matrix: one piece in place, or `n` pieces in row order in device memory
struct MuSource {
  int n;
  const MuPiece *pieces;
  MuPiece one;
};

// the value stored at (row, key) of the source; `keep` where there is none (the host checked the pattern: never)
__device__ __forceinline__ double mu_lookup(const MuSource &src, int row, int key, double keep) {
  const MuPiece *P = &src.one;
  if (src.n > 1) {                     // the last piece that starts at or before `row`
    int lo = 0, hi = src.n - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (src.pieces[mid].row0 <= row) lo = mid; else hi = mid - 1;
    }
    P = src.pieces + lo;
  }
  const int rl = row - P->row0;
  if (rl < 0 || rl >= P->rows) return keep;
  int lo = P->rowptr[rl], hi = P->rowptr[rl + 1];
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int c = P->col[mid];
    if (c == key) return P->val[mid];
    if (c < key) lo = mid + 1; else hi = mid;
  }
  return keep;
}

// slot (r, c) of a target whose rows start at global row `row0`: the searched (row, key)
template <bool TRANSPOSED>
__device__ __forceinline__ double mu_value(const MuSource &src, int r, int c, int row0, double keep) {
  return TRANSPOSED ? mu_lookup(src, c, r + row0, keep) : mu_lookup(src, r, c, keep);
}

// CSR-shaped targets (CSR(A) itself, a column slab): one wave per row, as scale_csr_kernel
template <bool TRANSPOSED>
__global__ __launch_bounds__(TPB) void mu_rows_kernel(int rows, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                      double *__restrict__ val, int row0, MuSource src, int skip_long) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int r = blockIdx.x * (TPB / WAVE) + threadIdx.x / WAVE;
  if (r >= rows) return;
  const int k0 = rowptr[r], k1 = rowptr[r + 1];
  if (skip_long && k1 - k0 > skip_long) return;      // mu_long_kernel takes those rows chunk by chunk
  for (int k = k0 + lane; k < k1; k += WAVE) val[k] = mu_value<TRANSPOSED>(src, r, col[k], row0, val[k]);
}

// rows beyond the long-row threshold: one workgroup per LONG_CHUNK entries, as scale_long_kernel
template <bool TRANSPOSED>
__global__ __launch_bounds__(TPB) void mu_long_kernel(const int *__restrict__ rowptr, const int *__restrict__ col,
                                                      double *__restrict__ val, const int *__restrict__ chunk_row,
                                                      const int *__restrict__ chunk_off, int row0, MuSource src) {
  const int r = chunk_row[blockIdx.x];
  const int kb = rowptr[r] + chunk_off[blockIdx.x];
  const int ke = min(kb + LONG_CHUNK, rowptr[r + 1]);
  for (int k = kb + threadIdx.x; k < ke; k += TPB) val[k] = mu_value<TRANSPOSED>(src, r, col[k], row0, val[k]);
}

// the sweep's tile-major copy: one wave per wave-row-block, walking its steps, as scale_tiled_kernel
template <bool TRANSPOSED>
__global__ __launch_bounds__(TPB) void mu_tiled_kernel(const int2 *__restrict__ wave_rows, const int *__restrict__ step_ptr,
                                                       const int *__restrict__ wave_step_off,
                                                       const int *__restrict__ step_tile,
                                                       const int *__restrict__ wg_step_off, int nwaves, int tile_shift,
                                                       const unsigned *__restrict__ pk, double *__restrict__ tv, int row0,
                                                       MuSource src) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = blockIdx.x * (TPB / WAVE) + threadIdx.x / WAVE;
  if (w >= nwaves) return;
  const int g = w / TW_WPB;
  const int nst = wg_step_off[g + 1] - wg_step_off[g];
  const int *stile = step_tile + wg_step_off[g];
  const int *sp = step_ptr + wave_step_off[w];
  const int r0 = wave_rows[w].x;
  const unsigned cmask = (1u << tile_shift) - 1u;
  for (int st = 0; st < nst; ++st) {
    const int tile = stile[st];
    for (int k = sp[st] + lane; k < sp[st + 1]; k += WAVE) {
      const unsigned p = pk[k];
      const int r = r0 + (int)(p >> tile_shift);
      const int c = tile + (int)(p & cmask);      // step_tile holds the tile's first column
      tv[k] = mu_value<TRANSPOSED>(src, r, c, row0, tv[k]);
    }
  }
}

// *bad = 1 when a row's column indices do not ascend strictly (one wave per row; reads only)
template <int UNUSED>
__global__ __launch_bounds__(TPB) void mu_ascending_kernel(int rows, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                           int *__restrict__ bad) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int r = blockIdx.x * (TPB / WAVE) + threadIdx.x / WAVE;
  if (r >= rows) return;
  const int k0 = rowptr[r], k1 = rowptr[r + 1];
  for (int k = k0 + 1 + lane; k < k1; k += WAVE)
    if (col[k] <= col[k - 1]) *bad = 1;
}

}  // namespace
