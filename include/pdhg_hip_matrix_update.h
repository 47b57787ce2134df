/* pdhg_hip_matrix_update.h -- new matrix values on a live handle whose sparsity pattern is kept.
 *
 * An addition to pdhg_hip.h and pdhg_hip_resolve.h (ABI version 11, unchanged: this entry point only adds).  The
 * re-solve calls of pdhg_hip_resolve.h keep a handle across solves whose VECTORS change.  Half of the callers those
 * calls were built for also get new matrix ENTRIES in the same places: a model-predictive controller with linearised,
 * time-varying dynamics, sequential LP / QP (the same Jacobian pattern in every outer iteration), a portfolio frontier
 * whose covariance is estimated again, scenario models whose coefficients are sampled again.  Layout construction, the
 * host builders, the create-time timing of sweep variants and every allocation depend on the pattern only, so such a
 * caller keeps the handle too:
 *
 *   create the handle, set Q, retain, rescale     once
 *   update the matrix values                      new entries of A (and Q) in the order of the create call, all four vectors
 *   rescale                                       exactly as after create
 *   warm start, step and check                    as before
 *
 * Bitwise contract.  After the call the handle holds, bit for bit, in every device array of every layout of A, A', Q
 * and Q' and in c, b, lb, ub, what a fresh handle holds that was created from the updated problem in the same
 * environment and given the retain call: the handle is NOT rescaled.  The retained record is reset (no steps, running
 * products 1.0; its capacity stays, so the rescale call that follows reuses it and the record does not grow from update
 * to update).  The iterates, the running sums and the restart point are left as they are -- they belong to the old
 * scaling, and the caller warm-starts, as every session solve does.  The originals stored for the evaluation are not
 * touched: the caller stores them again with the new rescaling factors, as every solve does.
 *
 * How.  CSR(A') is the create call's CSC narrowed to 32 bits, so the new values are its values as they are (one copy,
 * or one per row segment).  Every other copy holds the same entries in another order -- CSR(A), the long-row chunks,
 * the column slabs, the sweep's tile-major copy, the sliced jagged copies -- and takes each entry's value by a binary
 * search in an ascending run: CSR(A) from the row of CSR(A') that is the entry's column, the derived copies from the
 * entry's row of the matrix's own refreshed CSR.  No permutation and no other per-nonzero array stays on the handle:
 * a handle that never makes this call has the memory, the launches and the bits it had before this header existed.
 *
 * The searches need columns whose row indices ascend strictly.  pdhg_create also accepts columns that are unsorted or
 * hold duplicate entries; a handle created from such columns is refused here (-1).  That is found by one read-only pass
 * over the column indices, made by a handle's first update and remembered: the one refusal that launches anything.
 *
 * Handle kinds.  Plain handles (those held as row segments included) and fleet members.  Shard groups are refused;
 * batch handles and batch members are refused too: their layouts are lent between handles, and a batch takes new values
 * for all its members at once through the call that pdhg_hip_batch_matrix_update.h declares.
 */
#ifndef PDHG_HIP_MATRIX_UPDATE_H_
#define PDHG_HIP_MATRIX_UPDATE_H_

#include "pdhg_hip_resolve.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nzval (nnz): the constraint matrix's values in the order of the nzval given to the create call.  q_nzval (q_nnz): the
 * objective matrix's, in the order given to pdhg_set_objective_matrix; 0 / NULL on a handle without one.  c (n), b (m),
 * lb (n), ub (n): all four, in the space of the create call.
 *
 * Refused with -1 and a message, nothing launched or written, the handle usable as before: a NULL handle; no
 * pdhg_resolve_retain before; nnz or q_nnz other than what the handle was built with; a NULL nzval or vector; q_nzval
 * on a handle without Q, or Q present and q_nzval NULL (the call cannot change the class of the problem: the caller
 * keeps an all-zero Q away, which pdhg_set_objective_matrix would have treated as an LP); the handle kinds above.
 * Returns with the handle's stream idle. */
int pdhg_update_matrix_values(pdhg_handle *h, int64_t nnz, const double *nzval, int64_t q_nnz, const double *q_nzval,
                              const double *c, const double *b, const double *lb, const double *ub);

#ifdef __cplusplus
}
#endif
#endif /* PDHG_HIP_MATRIX_UPDATE_H_ */
