/* pdhg_hip_resolve.h -- re-solves on a live handle: new problem vectors in place, warm starts.
 *
 * An addition to pdhg_hip.h (ABI version 11, unchanged: these entry points only add).  The users of a first-order LP / QP
 * solver solve the same matrix again and again with other vectors, starting near the last answer: a model-predictive
 * controller with a new right-hand side every tick, branch-and-bound nodes that differ in a few bounds, scenario sets,
 * regularization paths.  The matrix copies, the layouts and the diagonal rescaling factors of a handle depend on the
 * constraint and objective matrices only, so such a caller keeps the handle:
 *
 *   create the handle, retain, rescale   once
 *   update the problem vectors           new c / b / lb / ub, in the space in which the create call took them
 *   warm start                           a starting point in that space (or zeros), everything else as on a fresh handle
 *   step and check                       as before
 *
 * Bitwise contract.  After an update the working vectors are, bit for bit, those of a fresh handle created from the
 * updated problem and rescaled with the same parameters: the rescaling rounds once per step and vector
 * (c = c / d, lb = lb * d, ub = ub * d, b = b / e), so the update replays the recorded steps one by one -- one division
 * by the cumulative factor would give other bits.  After a warm start at a point the handle is in the state of a fresh
 * handle given that point (scaled on the host by the cumulative factors) through the set-current call.
 *
 * Memory.  Retention is opt-in because the record is step-major in device memory, 8 * S * (n + m) bytes for S applied
 * steps (the per-step factors are needed, not only their product) plus 8 * (n + m) for the running products and two
 * staging buffers of 8 * (3 n + m) bytes, one of them pinned host memory.  Twelve steps (ten Ruiz passes, the L2 pass,
 * Pock-Chambolle) on a 10M x 10M problem are 1.9 GB.  Without the retain call nothing is recorded, and the rescaling
 * issues exactly the launches it always did.
 *
 * Handle kinds.  Plain handles (those held as row segments included: their vectors are whole) and fleet members are
 * supported.  Batch handles, batch members and shard groups are refused with -1 and a message, before any device work.
 *
 * Every function returns 0 on success; otherwise the last-error text of pdhg_hip.h says why.
 */
#ifndef PDHG_HIP_RESOLVE_H_
#define PDHG_HIP_RESOLVE_H_

#include "pdhg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* To be called before the handle is rescaled (and after a QP's objective matrix is set).  From then on every rescaling
 * step appends its column and row factors to a record on the handle, and the running products are kept with them -- the
 * same bits as the arrays the rescale call returns.  A second call is a no-op.  A handle that is never rescaled after
 * this call (the caller rescaled on the host) has an empty record: updates and warm starts are then copies. */
int pdhg_resolve_retain(pdhg_handle *h);

/* New c (n), b (m), lb (n), ub (n) in the space in which the handle was created; NULL: that vector stays as it is.
 * One upload of what was given through a pinned staging buffer owned by the handle, one launch that writes the working
 * vectors by replaying the recorded steps in order.  A pending lazy accept is settled first; afterwards the evaluation
 * caches, a fleet member's stored check results and (when a bound was given) the compact views of lb / ub are dropped
 * and rebuilt.  The originals stored for the evaluation are not touched: the caller stores the updated originals again,
 * as every solve does.  Refused if the retain call was not made.  Returns with the handle's stream idle. */
int pdhg_update_problem_vectors(pdhg_handle *h, const double *c, const double *b, const double *lb, const double *ub);

/* Start from the point x (n), y (m) given in create space; NULL: zeros.  One launch sets x_s = x * cum_d and
 * y_s = y * cum_e and empties what a fresh handle has empty: the running sums, their counts and weights, the alternates
 * of the paired average update, a pending lazy accept (discarded, not settled), the saved restart point, a QP's kept
 * Q x.  Then A'y by the handle's own product; with y == NULL the product is filled with +0.0 instead, which is what a
 * fresh handle holds (the product of a zero vector can leave -0.0 in a column of negative entries).  The point is not
 * projected onto the bounds: the first step does that.  Refused if the retain call was not made. */
int pdhg_warm_start(pdhg_handle *h, const double *x, const double *y);

/* The fleet forms: each argument is an array of K pointers (K = the fleet's members, in order of addition), or NULL.
 * All members' vectors are packed into one pinned table, uploaded once, and ONE launch does the work of every member,
 * whatever its size: the work items are (member, chunk of 1024 elements).
 *
 * Update: a NULL array or a NULL entry means "keep".  A member whose bounds were given has its compact bound views
 * marked stale instead of rebuilt (a rebuild synchronizes and allocates; K of them would undo the shared launch): they
 * are rebuilt where they are next read -- before a primal-step launch or a trial graph's primal node, or when the layout
 * is described.  The one-workgroup kernels read the dense arrays and never need them. */
int pdhg_fleet_update_problem_vectors(pdhg_handle *fleet, const double *const *c, const double *const *b,
                                      const double *const *lb, const double *const *ub);

/* Warm start: a member whose x and y entries are both NULL is left exactly as it is; with one entry given the other
 * means zeros.  Both ARRAYS NULL: every member starts from zeros.  A'y of the members of the fleet's check class
 * (n + m <= 4096, rows of at most 256 entries) is computed in the shared launch of the fleet's point products, which is
 * bit for bit the member's own product; every other member is served by its own product inside the call. */
int pdhg_fleet_warm_start(pdhg_handle *fleet, const double *const *x, const double *const *y);

/* out[0] shared re-solve launches so far (one per fleet update or fleet warm start that carried a member),
 * out[1] members carried by the last such call, out[2] members of the last warm start given a product of their own,
 * out[3] lazy rebuilds of bound views so far. */
int pdhg_fleet_resolve_info(pdhg_handle *fleet, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* PDHG_HIP_RESOLVE_H_ */
