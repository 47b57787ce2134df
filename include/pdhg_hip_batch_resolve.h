/* pdhg_hip_batch_resolve.h -- re-solves of a batch on its handle: new problem vectors in place, warm starts.
 *
 * An addition to pdhg_hip.h and pdhg_hip_resolve.h (ABI version 11, unchanged: these entry points only add).  A batch
 * (pdhg_create_batch) is K problems over one constraint matrix -- and one objective matrix -- that differ in c, b and
 * the bounds: the ticks of a model-predictive controller with K right-hand sides, personalized PageRank, a
 * regularization path, a portfolio frontier.  These callers solve again and again, starting near the last answer, and
 * everything a create and a rescale do depends on the matrices only.  Such a caller keeps the batch:
 *
 *   create the batch, set the objective matrix, retain, rescale     once
 *   update the members' problem vectors                             in the space in which the create call took them
 *   warm start the members                                          points in that space (or zeros)
 *   step and check                                                  as before
 *
 * Bitwise contract.  After an update every carried member's working vectors are, bit for bit, those of the member of a
 * fresh batch created from the updated problems and rescaled with the same parameters.  After a warm start a carried
 * member is in the state of a fresh member given that point (scaled on the host by the cumulative factors) through the
 * set-current call of pdhg_hip.h, its product A'y included.
 *
 * Memory.  The rescaling factors depend on the matrix, so the record of the applied steps and the running products are
 * kept ONCE, on the batch handle: 8 * S * (n + m) + 8 * (n + m) bytes for S steps, not K times that.  The two staging
 * buffers (one pinned) hold K * (3 n + m) doubles and a head of a few KiB.
 *
 * The calls of pdhg_hip_resolve.h for one handle keep refusing a batch handle and a batch member.
 *
 * Every function returns 0 on success; otherwise the last-error text of pdhg_hip.h says why.  A refusal launches nothing.
 */
#ifndef PDHG_HIP_BATCH_RESOLVE_H_
#define PDHG_HIP_BATCH_RESOLVE_H_

#include "pdhg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* To be called on the batch handle before it is rescaled (and after the objective matrix is set).  From then on every
 * rescaling step appends its column and row factors to one record on the batch handle, shared by the members.  A second
 * call is a no-op.  Anything that is not a batch handle is refused with -1. */
int pdhg_batch_resolve_retain(pdhg_handle *batch);

/* New c (n), b (m), lb (n), ub (n) of the members: each argument is NULL or an array of K pointers (K = the batch's
 * members); a NULL array or a NULL entry means "keep".  All given vectors are packed into one pinned buffer, uploaded
 * once, and ONE launch replays the recorded steps on every carried member: the record is read once per tile of four
 * members, not once per member.  A carried member's pending lazy accept is settled first; a member whose bounds were
 * given has its compact bound views marked stale and rebuilt where they are next read (the batched trial reads the
 * dense arrays).  The batch handle's own c / b / lb / ub, which no solve reads, stay as they are, and so do the
 * originals stored for the evaluation: the caller stores the updated originals again, as every solve does.
 * Refused if the retain call was not made.  Returns with the batch's stream idle. */
int pdhg_batch_update_problem_vectors(pdhg_handle *batch, const double *const *c, const double *const *b,
                                      const double *const *lb, const double *const *ub);

/* Starting points x (n), y (m) of the members in create space: arrays of K pointers.  Both ARRAYS NULL: every member
 * starts from zeros.  Otherwise a member whose x and y entries are both NULL is left exactly as it is, and with one
 * entry given the other means zeros.  One upload and one launch set x_s = x * cum_d, y_s = y * cum_e of every carried
 * member and empty what a fresh member has empty (the running sums, their counts and weights, a pending lazy accept,
 * the saved restart point, a QP's kept Q x).  A'y of every member given a y is computed in ONE batched product when
 * every row of A' lies within the row order's sequential limit (2048 entries in strict order, 256 in relaxed order),
 * where the batched row sum is the member's own product bit for bit; otherwise each such member runs its own product.
 * A member without y gets +0.0.  Refused if the retain call was not made. */
int pdhg_batch_warm_start(pdhg_handle *batch, const double *const *x, const double *const *y);

/* out[0] shared re-solve launches so far (one per update; one per warm start for the points and one more when the
 * batched product ran), out[1] members carried by the last update or warm start, out[2] members of the last warm start
 * given a product of their own, out[3] 1 if the last warm start ran the batched product. */
int pdhg_batch_resolve_info(pdhg_handle *batch, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* PDHG_HIP_BATCH_RESOLVE_H_ */
