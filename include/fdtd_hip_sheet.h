/* fdtd_hip_sheet.h — conducting sheets (finite-conductivity metal as a surface impedance) on top of fdtd_hip.h.
 *
 * Kept out of fdtd_hip.h on purpose: that header is the ABI every backend (the CPU oracle included) exports in full, and
 * FDTD_ABI_VERSION stays what it is.  Only libfdtd_hip.so exports these two symbols.
 *
 * Model (fdtd-solver-antennas_amd/sheet.py): the surface admittance of a metal face is fitted as
 *   Y_s(jw) ~= G0 + sum_k c_k / (jw + p_k),   G0, c_k >= 0,
 * and discretised with alpha_k = exp(-p_k dt), b_k = c_k (1 - alpha_k) / p_k.  The implicit part,
 * scale_e * (G0 + sum_k b_k), is folded into the conductance of the sheet edges when the operator is built (the lumped-edge
 * overrides of fdtd_build_operator).  What remains is a sparse correction, applied once per timestep after the E phase
 * (update, Mur passes, sources, V-probes, V-DFT) and before the H update, per sheet edge e and in this fp32 order:
 *
 *   S      = sum_k alpha_k * i_k            (k ascending, starting from 0.0f)
 *   V_new  = V - vi_e * S
 *   i_k    = alpha_k * i_k + bs_k * (0.5f * (V_new + v_prev))      bs_k = scale_e * b_k of the edge's class
 *   v_prev = V_new
 *
 * A context with sheets steps under the two-launch schedule (three with Mur faces) plus one k_sheet launch per timestep;
 * forcing FDTD_FLAG_KERNEL_WAVEFRONT or FDTD_FLAG_KERNEL_RESIDENT returns FDTD_E_UNSUPPORTED, and so does world > 1.
 * fdtd_half_step(ctx, FDTD_PHASE_E) applies the correction too.  Branch currents and v_prev start at zero (the fields are
 * zero before the first step); fdtd_set_field does not touch them.
 *
 * The order above holds for any edge set this call accepts, under fdtd_run as under fdtd_half_step: a V-probe whose cell sits
 * on the node of a sheet edge is sampled in a launch of its own in front of the correction (k_post) instead of in the probe
 * blocks of update_H, and a sheet edge on the node plane of an enabled Mur face makes the Mur apply pass a launch of its own
 * (three launches per timestep), so that the correction reads the face's final voltage.  (The scene layer places sheets off
 * probe lines and two planes inside Mur faces; neither case costs a context built by it anything.)
 *
 * Lumped R-L-C elements — a two-state branch per edge, complex pole pairs included — are fdtd_hip_lumped.h.
 */
#ifndef FDTD_HIP_SHEET_H
#define FDTD_HIP_SHEET_H

#include <stdint.h>
#include "fdtd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FDTD_SHEET_MAX_K 8

/* n sheet edges: global flat node index idx[e] (as fdtd_add_source), component comp[e] (0..2), the edge's full vi
 * coefficient vi[e] (fdtd_get_operator), class cls[e] in [0, ncls).  alpha and b are [ncls][K] (K in 1..FDTD_SHEET_MAX_K):
 * b holds scale_e * b_k of the class, the factor the update multiplies by.  No edge twice.  Call after the operator is set
 * and before the first timestep; a second call replaces the set (n = 0 removes it). */
int fdtd_sheet_set(fdtd_ctx* ctx, int n, const int64_t* idx, const int8_t* comp, const float* vi, const int32_t* cls,
                   int ncls, int K, const float* alpha, const float* b);

/* State of the sheet edges, for tests: v_prev [n] and the branch currents i_branch [K][n] (either may be NULL). */
int fdtd_sheet_get(fdtd_ctx* ctx, float* v_prev, float* i_branch);

#ifdef __cplusplus
}
#endif
#endif
