/* fdtd_hip_traffic.h — which memory-traffic shortcuts a context of libfdtd_hip.so took.
 *
 * Kept out of fdtd_hip.h on purpose, as fdtd_hip_sheet.h is: that header is the ABI every backend (the CPU oracle included) exports
 * in full, fdtd_schedule_info has no free slot, and FDTD_ABI_VERSION stays what it is.  Only libfdtd_hip.so exports this symbol.
 *
 * Two shortcuts remove bytes the result does not depend on; neither changes a field value:
 *
 *  * Inert CPML indices.  fdtd_set_cpml trims, per axis and per side (E-located / H-located tables), both ends of the two slot
 *    ranges while b == 0, c == 0 and 1 / kappa == 1.  Along y and z the update kernels treat a trimmed index as "no layer here".
 *    ($FDTD_PSI_ACTIVE=0 keeps the whole ranges active.)
 *  * Class rows.  A packed class operator (one byte per cell) whose distinct (k, j) rows fit in 1 MiB is read as one row offset per
 *    (k, j) plus the table of distinct rows.  ($FDTD_CLASS_ROWS=0 keeps the per-cell bytes.)
 */
#ifndef FDTD_HIP_TRAFFIC_H
#define FDTD_HIP_TRAFFIC_H

#include <stdint.h>
#include "fdtd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* skipped[2 * axis + side]: inert indices of this context's slab that the kernels skip (axis 0..2 = x, y, z; side 0 = E-located,
 * 1 = H-located; x is never trimmed: 0).  class_rows: distinct class rows in use (0: per-cell form).  bytes_saved: the resulting
 * estimate of bytes per timestep that no longer move — 16 B per cell of a skipped plane or row (two psi arrays, read and written),
 * and the class bytes less the row offsets. */
int fdtd_traffic_info(fdtd_ctx* ctx, int32_t skipped[6], int32_t* class_rows, int64_t* bytes_saved);

#ifdef __cplusplus
}
#endif
#endif
