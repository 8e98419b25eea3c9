/* fdtd_hip_aniso.h — anisotropic dielectrics (diagonal permittivity and conductivity tensors) on top of fdtd_hip.h.
 *
 * Kept out of fdtd_hip.h for the reason fdtd_hip_sheet.h is: that header is the ABI every backend (the CPU oracle included)
 * exports, and the oracle does not build this operator — it is handed the host arrays instead (ecoperator.build_operator).
 * Exported by libfdtd_hip.so only; not part of FDTD_ABI_VERSION.
 *
 * The model (ecoperator.py is the specification): the equivalent-circuit operator holds one (vv, m) pair per EDGE, and an edge has
 * a direction.  An edge of component c takes the area-weighted four-cell means of eps_r[c] and kappa[c]; nothing else of
 * fdtd_build_operator changes — summation order, the float64 expressions for x, vv and m, slab windows, overrides, the class
 * numbering and the three forms (packed classes, per-edge classes, raw).  Hence component c of the result is, bit for bit, component
 * c of what fdtd_build_operator gives for (eps_r[c], kappa[c]); three equal arrays give fdtd_build_operator's bits and form.  The
 * step loop reads the operator as before: no schedule, step kernel or correction knows about the tensor.
 */
#ifndef FDTD_HIP_ANISO_H
#define FDTD_HIP_ANISO_H

#include "fdtd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The arguments of fdtd_build_operator with three cell arrays each: eps_r[c], kappa[c] double [nz-1][ny-1][nx-1] of the GLOBAL grid,
 * read by the edges of component c (0 x, 1 y, 2 z).  Pointers may coincide (an array shared by several axes is uploaded once).
 * Returns FDTD_OK or a negative FDTD_E_* code (message: fdtd_last_error(ctx)). */
int fdtd_build_operator_axes(fdtd_ctx* ctx, const double* dx, const double* dy, const double* dz, const double* const eps_r[3],
                             const double* const kappa[3], const uint8_t* pec, double eps0, int n_over, const int64_t* over_edge,
                             const int8_t* over_comp, const float* over_vv, const float* over_m, const float* emet, const float* hmet,
                             int prefer_classes);

#ifdef __cplusplus
}
#endif
#endif
