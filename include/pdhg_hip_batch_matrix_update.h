/* pdhg_hip_batch_matrix_update.h -- new matrix values for a batch whose sparsity pattern is kept.
 *
 * An addition to pdhg_hip.h, pdhg_hip_batch_resolve.h and pdhg_hip_matrix_update.h (ABI version 11, unchanged: this
 * entry point only adds).  A batch's members share one constraint matrix -- and one objective matrix -- whose layouts
 * live on the batch handle and are lent to the members.  The callers a batch was built for are the ones whose matrix
 * moves between ticks: a model-predictive controller linearised again around a new trajectory with K right-hand sides,
 * sequential LP / QP over a scenario set, a frontier over a covariance that is estimated again.  Layout construction,
 * the create-time timing, every allocation and the K member creates depend on the pattern only, so such a caller keeps
 * the batch:
 *
 *   create the batch, set the objective matrix, retain, rescale     once
 *   update the matrix values                                        new entries of A (and Q), the K members' four vectors
 *   rescale the batch handle                                        exactly as after create
 *   warm start the members, step and check                          as before
 *
 * Bitwise contract.  After this call and the pdhg_rescale that must follow it, every device array of every layout of A,
 * A', Q and Q', every member's c, b, lb, ub and the batch handle's own four vectors hold, bit for bit, what a fresh batch
 * holds that was created from the updated problems in the same environment, retained and rescaled with the same
 * parameters.
 *
 * How.  The values are placed as pdhg_update_matrix_values places them (one upload into CSR(A'), every other copy by
 * search; the members' layouts are the same device arrays).  The members' raw vectors are staged on the device, in the
 * retained record's staging buffer, and the batch is marked "members awaiting the rescale".  pdhg_rescale on a marked
 * batch records its steps as always, leaves the members' vectors alone step by step, and ends with ONE launch that
 * replays the whole record on the staged vectors of all K members (the launch pdhg_batch_update_problem_vectors makes):
 * one launch instead of K per rescaling step.  A rescale of zero steps leaves the raw vectors in the members.  Then the
 * mark is cleared.
 *
 * While the mark is set every entry point on the batch or on a member -- trial, accept, evaluation, warm start, vector
 * update, another update of the matrix values -- is refused with -1 and a message that says to rescale the batch first.
 * pdhg_rescale on the batch handle, pdhg_destroy and the info calls (pdhg_batch_resolve_info, pdhg_batch_check_info,
 * pdhg_batch_member) proceed.
 *
 * A batch that never makes this call has the memory, the launches and the bits it had before this header existed.
 */
#ifndef PDHG_HIP_BATCH_MATRIX_UPDATE_H_
#define PDHG_HIP_BATCH_MATRIX_UPDATE_H_

#include "pdhg_hip_batch_resolve.h"
#include "pdhg_hip_matrix_update.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nzval (nnz): the constraint matrix's values in the order of the nzval given to pdhg_create_batch.  q_nzval (q_nnz): the
 * objective matrix's, in the order given to pdhg_batch_set_objective_matrix; 0 / NULL on an LP batch.  c, b, lb, ub: tables
 * of K pointers as pdhg_batch_update_problem_vectors takes them; here every entry is needed, and every vector is raw, in
 * the space of pdhg_create_batch.
 *
 * Refused with -1 and a message, nothing launched or written, the batch usable as before: a NULL handle or one that is
 * not a batch; no pdhg_batch_resolve_retain before; nnz or q_nnz other than what the batch was built with; a NULL nzval,
 * table or table entry; q_nzval on an LP batch, or a QP batch and q_nzval NULL; a batch that still awaits the rescale of
 * an earlier call.  A batch created from columns whose row indices do not ascend strictly is refused after one read-only
 * pass over the pattern, made by the batch's first call and remembered.
 *
 * A device error after the call has begun to place values leaves new raw values under vectors of the old scaling: the
 * call returns the error, and from then on every call on the batch and its members, the rescale included, is refused --
 * only pdhg_destroy proceeds.
 *
 * pdhg_batch_resolve_info afterwards: the replay launch is counted by the pdhg_rescale that makes it, with out[1] = K.
 * Returns with the batch's stream idle. */
int pdhg_batch_update_matrix_values(pdhg_handle *batch, int64_t nnz, const double *nzval, int64_t q_nnz, const double *q_nzval,
                                    const double *const *c, const double *const *b, const double *const *lb,
                                    const double *const *ub);

#ifdef __cplusplus
}
#endif
#endif /* PDHG_HIP_BATCH_MATRIX_UPDATE_H_ */
