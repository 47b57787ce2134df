/* pdhg_hip_batch_checks.h -- a batch's check products and evaluations in shared launches.
 *
 * An addition to pdhg_hip.h (ABI version 11, unchanged: these entry points only add).  The members of a batch
 * (pdhg_create_batch) share the constraint matrix -- and the objective matrix -- and their trials read it once for all
 * of them.  Between the trials every member checks: a termination evaluation (pdhg_eval_point) and up to three rounds of
 * trust-region problems, each of which begins with A x, A' y (and Q x) at one of the member's three points.  Member by
 * member that is up to 3 K reads of the shared matrix per product and K second-stage launches with K host round trips.
 * The calls here take those products for all members from one read of the matrix per point kind, and the evaluations of
 * all members in four launches.  Nothing else changes: each member's own calls follow as before and find the results.
 *
 * Bitwise contract.  What a call leaves in a member -- the product caches of a point, the materialised average, the
 * stored evaluation -- is, bit for bit, what the member's own pdhg_eval_point / pdhg_trust_region_bound(s) would have
 * computed in its place.  The packed average is divided as the member divides it; a batched row sum is one lane adding
 * the row left to right from 0.0, which is the member's own order for every row within the row order's sequential limit
 * (2048 entries in strict order, 256 in relaxed order); the evaluation kernels run the member kernels' bodies on the
 * member's own grid and partials, and the second stage is the member's, one workgroup per member.
 * A product whose matrix has a row beyond that limit (the batch splits such rows into chunks, another summation order) is
 * taken by every member's own product launch inside the call, for that product only; the other products of the same pass
 * stay batched.  The trust-region searches themselves stay per member: a member's search is grouped by its own grid, and
 * a cross-member search in another grouping could not return the member's bits.  They gain their point products, which
 * arrive cached.
 *
 * What is forgotten when.  The product caches are keyed as the member keys them: CURRENT and AVERAGE by the member's
 * state (any step, restart, update or warm start moves it), RESTART by the restart point and the matrix.  A stored
 * evaluation answers the member's pdhg_eval_point (and, through it, pdhg_distance_to_restart and pdhg_point_sumsq) only
 * for the same point and while the member's state, restart point and matrix are those of the call; it is dropped by
 * pdhg_set_original_problem on the member, by pdhg_batch_update_problem_vectors and pdhg_batch_warm_start for the members
 * they touch, and by pdhg_batch_set_objective_matrix.
 *
 * Refusals.  Each call returns -1 with the last-error text of pdhg_hip.h, before any launch or write: a handle that is
 * not a batch handle; a member index outside 0 .. K-1; a point that is not one of PDHG_POINT_CURRENT / AVERAGE / RESTART;
 * a count outside 1 .. 3 * 32; PDHG_POINT_AVERAGE for a member whose average is empty ("average is empty");
 * pdhg_batch_eval_points for a member without pdhg_set_original_problem.
 */
#ifndef PDHG_HIP_BATCH_CHECKS_H_
#define PDHG_HIP_BATCH_CHECKS_H_

#include "pdhg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A x, A' y and, on a QP batch, Q x at point[i] of member[i] for i < count (1 .. 96 items) into that member's product
 * cache of that point, with the cache keys set: the member's own calls at that point then launch no product.  An item
 * whose cache is fresh already is skipped.  What is pending on the named members (a lazy accept) is settled first.  One
 * pass per point kind, so at most three: a pack kernel over (element, member) writes the points member-interleaved --
 * for AVERAGE it divides the running sums and stores the average in the member as well -- then one plain batched product
 * per matrix writes through a table of the members' cache buffers. */
int pdhg_batch_point_products(pdhg_handle *batch, int count, const int *member, const int *point);

/* pdhg_eval_point(member k, points[k], out + 24 k) for every k < K with points[k] >= 0 (-1: the member is left alone and
 * its 24 values of out are not written).  The products as above; then the row quantities, the column quantities and the
 * three distance pairs of all carried members in three launches over (block, member), and one second-stage launch of one
 * workgroup per member that publishes each member's 28 result words into pinned memory, which the host reads without a
 * copy.  Every result is stored with its member, with what pdhg_eval_point keeps for pdhg_distance_to_restart and
 * pdhg_point_sumsq. */
int pdhg_batch_eval_points(pdhg_handle *batch, const int *points, double *out);

/* Counters since the batch was created: out[0] calls of the two functions above; out[1] items whose products (at least
 * one of them) rode a batched launch; out[2] items with a product served by the member's own launch (long rows);
 * out[3] items found cached; out[4] members carried by pdhg_batch_eval_points; out[5] pdhg_eval_point calls on members
 * answered from a stored result; out[6] pdhg_eval_point calls on members that had to launch although
 * pdhg_batch_eval_points had been called on the batch before (misses); out[7] kernel launches issued by the two calls. */
int pdhg_batch_check_info(pdhg_handle *batch, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* PDHG_HIP_BATCH_CHECKS_H_ */
