/* fdtd_hip_lumped.h — lumped R-L-C elements on mesh edges, on top of fdtd_hip.h.
 *
 * Kept out of fdtd_hip.h for the reason fdtd_hip_sheet.h is: that header is the ABI every backend (the CPU oracle included)
 * exports in full, and FDTD_ABI_VERSION stays what it is.  Only libfdtd_hip.so exports these two symbols.
 *
 * Model (fdtd-solver-antennas_amd/lumped.py): an element — R, L, C in parallel or in series — is a one-port with at most two
 * states x, discretised with the trapezoidal rule and driven by the edge's mean voltage Vm over the step:
 *   x' = Phi x + Gam Vm,     mean current  ibar = h.x + g0 Vm.
 * g0 (and a plain 1/R) is folded into the conductance of the edge, a plain C into its capacitance, when the operator is built
 * (the lumped-edge overrides of fdtd_build_operator).  What remains is a sparse correction, applied once per timestep after the
 * E phase (update, Mur passes, sources, V-probes, V-DFT / recorder), after the corrections of the Debye media and the
 * conducting sheets when the context has those, and before the H update — per element edge e, with the tables of the edge's
 * class, in this fp32 order (every statement one operation, no contraction):
 *
 *   p0 = h0*x0;  p1 = h1*x1;  S = p0 + p1
 *   q  = vi_e*S;  v = V - q
 *   s  = v + v_prev;  avg = 0.5f*s
 *   a = phi00*x0;  b = phi01*x1;  c = a + b;  d = gam0*avg;  x0' = c + d
 *   a = phi10*x0;  b = phi11*x1;  c = a + b;  d = gam1*avg;  x1' = c + d
 *   x0 = x0';  x1 = x1';  V = v;  v_prev = v
 *
 * A context with element edges steps under the two-launch schedule (three with Mur faces) plus one k_lumped launch per
 * timestep; forcing FDTD_FLAG_KERNEL_WAVEFRONT or FDTD_FLAG_KERNEL_RESIDENT returns FDTD_E_UNSUPPORTED, and so do world > 1,
 * the p2p transport and linked contexts.  fdtd_half_step(ctx, FDTD_PHASE_E) applies the correction too.  States and v_prev
 * start at zero (the fields are zero before the first step); fdtd_set_field does not touch them.
 *
 * The order above holds for any edge set this call accepts, under fdtd_run as under fdtd_half_step, by the rules the sheets
 * have: a V-probe whose cell sits on the node of an element edge is sampled in a launch of its own in front of the corrections,
 * and an element edge on the node plane of an enabled Mur face makes the Mur apply pass a launch of its own.
 */
#ifndef FDTD_HIP_LUMPED_H
#define FDTD_HIP_LUMPED_H

#include <stdint.h>
#include "fdtd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n element edges: global flat node index idx[e] (as fdtd_add_source), component comp[e] (0..2), the edge's full vi
 * coefficient vi[e] (fdtd_get_operator), class cls[e] in [0, ncls).  Per class phi [ncls][2][2] (row-major: phi00, phi01,
 * phi10, phi11), gam [ncls][2], h [ncls][2]; a one-state class leaves its second row and column at zero.  No edge twice.  Call
 * after the operator is set and before the first timestep; a second call replaces the set (n = 0 removes it). */
int fdtd_lumped_set(fdtd_ctx* ctx, int n, const int64_t* idx, const int8_t* comp, const float* vi, const int32_t* cls, int ncls,
                    const float* phi, const float* gam, const float* h);

/* State of the element edges, for tests: v_prev [n] and the states x [2][n] (either may be NULL). */
int fdtd_lumped_get(fdtd_ctx* ctx, float* v_prev, float* x);

#ifdef __cplusplus
}
#endif
#endif
