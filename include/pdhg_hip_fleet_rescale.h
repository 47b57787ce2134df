/* pdhg_hip_fleet_rescale.h -- the rescaling of a fleet's members in one shared launch.
 *
 * An addition to pdhg_hip.h (ABI version 11, unchanged: these entry points only add).  A fleet shares launches for its
 * members' steps, checks, vector updates and warm starts; pdhg_rescale and pdhg_matrix_max_abs were the one device
 * phase its members still took in turn -- about a dozen launches, a view rebuild with its round trip per step and eight
 * allocations per member, for microseconds of device work.  pdhg_fleet_rescale takes every member named through
 * pdhg_rescale followed by pdhg_matrix_max_abs inside one call:
 *
 *   a member of the one-workgroup class     rides in ONE launch of fleet_rescale_kernel, one workgroup per member
 *   every other member                      is served by its own pdhg_rescale and pdhg_matrix_max_abs inside the same
 *                                           call, member after member (pdhg_fleet_take_steps_adaptive's convention)
 *
 * The class: one plain handle (no shard group, not profiled) whose resident copies of A, A' (and Q, Q') are plain CSR
 * arrays -- no row segments, no tiled copy, no column slabs, no sliced jagged copy, no row beyond the long-row
 * threshold -- with 1 <= n + m <= 4096 (four factor vectors of n + m doubles in one workgroup's LDS).  LPs and QPs alike.
 *
 * Bitwise contract.  Whatever the class, every device array of the member, the arrays returned, the retained record of
 * a member with pdhg_resolve_retain and its running products hold, bit for bit, what the member's own pdhg_rescale
 * with the same arguments leaves, and max |a| is pdhg_matrix_max_abs's.  The compact bound views of a carried member
 * are rebuilt where they are next read (the rule of pdhg_fleet_update_problem_vectors), once, instead of once per step.
 */
#ifndef PDHG_HIP_FLEET_RESCALE_H_
#define PDHG_HIP_FLEET_RESCALE_H_

#include "pdhg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pdhg_rescale and then pdhg_matrix_max_abs of member k, for every k with active[k] != 0 (active == NULL: every
 * member); the other members are left as they are, their versions included.  constraint_rescaling_out /
 * variable_rescaling_out: NULL, or K pointers of which each may be NULL (m / n doubles of member k);
 * matrix_max_abs_out: NULL or K doubles (entry k is written for an active member only).  With no step requested the
 * factors are ones, nothing is scaled and max |a| is still reported.
 *
 * Refused with -1 and a message, nothing launched or written: a NULL handle or one that is no fleet;
 * pock_chambolle_alpha outside [0, 2] when use_pock_chambolle; l_inf_ruiz_iterations < 0; an active member that is not
 * a usable handle.  Returns with the fleet's stream idle. */
int pdhg_fleet_rescale(pdhg_handle *fleet, const int *active /* K flags, NULL: all */,
                       int l_inf_ruiz_iterations, int l2_norm_rescaling, int use_pock_chambolle, double pock_chambolle_alpha,
                       double *const *constraint_rescaling_out, double *const *variable_rescaling_out /* K pointers, each may be NULL */,
                       double *matrix_max_abs_out /* K, may be NULL */);

/* out[0]: shared rescale launches so far; out[1], out[2]: members the last pdhg_fleet_rescale carried in its launch /
 * served by their own calls; out[3]: lazy rebuilds of bound views so far (pdhg_fleet_resolve_info's count). */
int pdhg_fleet_rescale_info(pdhg_handle *fleet, int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* PDHG_HIP_FLEET_RESCALE_H_ */
