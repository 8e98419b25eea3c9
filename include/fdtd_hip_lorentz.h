/* fdtd_hip_lorentz.h — resonant dielectrics (Lorentz and Drude poles) on top of fdtd_hip.h.
 *
 * Kept out of fdtd_hip.h on purpose, as fdtd_hip_dispersion.h is: that header is the ABI every backend (the CPU oracle included)
 * exports in full, and FDTD_ABI_VERSION stays what it is.  Only libfdtd_hip.so exports these two symbols.
 *
 * Model (fdtd-solver-antennas_amd/lorentz.py):
 *   eps(w) = eps_inf (1 + sum_k wp_k^2 / (w0_k^2 - w^2 + j w gamma_k)) - j kappa / (w eps0),   wp_k > 0, w0_k >= 0, gamma_k >= 0, K <= 4
 * (w0_k = 0: a Drude pole).  Each pole is a series R-L-C branch (R-L for a Drude pole) across the edge capacitance with, per unit
 * of the edge weight w_e [m] (the share of the edge's A~/l that lies in the medium, as for the Debye media),
 *   l_k = 1 / (eps0 eps_inf wp_k^2),   r_k = gamma_k l_k,   c_k = eps0 eps_inf wp_k^2 / w0_k^2,
 * and the two states x_k = (j_k, u_k): l dj/dt = v - r j - u, c du/dt = j; the branch current of the edge is w_e j_k.  The branch
 * is discretised as a series element of fdtd_hip_lumped.h is — trapezoidal rule driven by Vm = (V_new + V_prev) / 2:
 *   x_k' = Phi_k x_k + Gam_k Vm,   mean current per unit weight = h_k . x_k + g0_k Vm
 * — so it is passive and leaves the Courant limit alone.  g0_k is a conductance per unit weight: it is folded into the cells'
 * kappa when the operator is built (kappa_cell += sum_k g0_k, eps_cell = eps_inf), so the operator keeps its form.  What
 * remains is applied once per timestep AFTER the whole E phase (update, Mur passes, sources, V-probes, V-DFT / recorder) and the
 * Debye media's correction, BEFORE the conducting sheets' and the lumped elements' corrections and the H update — per
 * dispersive edge e (w_e != 0) of medium m, every statement one fp32 operation, no contraction:
 *
 *   S = 0.0f;   for k = 0 .. K-1:   p0 = h[m][k][0] * j_k;   p1 = h[m][k][1] * u_k;   s = p0 + p1;   S = S + s
 *   t      = w_e * S
 *   q      = vi_e * t
 *   V_new  = V - q
 *   s      = V_new + v_prev
 *   avg    = 0.5f * s
 *   for k = 0 .. K-1:   a = phi[m][k][0][0] * j_k;   b = phi[m][k][0][1] * u_k;   c = a + b;   d = gam[m][k][0] * avg;   j_k' = c + d
 *                       a = phi[m][k][1][0] * j_k;   b = phi[m][k][1][1] * u_k;   c = a + b;   d = gam[m][k][1] * avg;   u_k' = c + d
 *                       (both rows from the OLD j_k, u_k; products and sums separate: no fma)
 *   v_prev = V_new
 *
 * phi, gam and h arrive as fp32 tables (rounded from the host's float64 values).  A Drude pole leaves the second row and column
 * of its phi, gam[1] and h[1] at zero: its u_k stays 0.  Edges with w_e == 0 inside a box are left alone: V, j_k, u_k and v_prev
 * keep their bits.  Edges the operator holds at zero (vi_e == 0: the tangential edges of every grid face, edges in metal) are left
 * alone too, whatever their w_e: fdtd_lorentz_set treats them as w_e = 0, for the reasons fdtd_hip_dispersion.h gives (q is 0
 * there; and a medium may run into a Mur face under every schedule).
 *
 * Storage: per field component one dense box [z0, z1) x [y0, y1) x [x0, x1) of edges (node indices of the edges' lower ends),
 * laid out like the field arrays (x fastest); the library widens x0 down and x1 up to multiples of 4, so one thread owns four
 * consecutive x-edges of a row and moves V, v_prev, w, vi and every state plane as 16-byte vectors.  States are
 * structure-of-arrays over (pole, state): plane 2 k holds j_k, plane 2 k + 1 holds u_k.
 *
 * A context with media steps under the two-launch schedule (three with Mur faces) plus one k_lorentz launch per timestep;
 * forcing FDTD_FLAG_KERNEL_WAVEFRONT or FDTD_FLAG_KERNEL_RESIDENT returns FDTD_E_UNSUPPORTED, and so do world > 1, the p2p
 * transport and linked contexts.  Because the correction follows the V-probes, fdtd_run samples those in a launch of their own
 * in front of it (k_post), as for Debye media.  fdtd_half_step(ctx, FDTD_PHASE_E) applies the correction too.  The states and
 * v_prev start at zero (the fields are zero before the first step); fdtd_set_field does not touch them.  A context without media
 * launches exactly what it launched before this header existed.
 */
#ifndef FDTD_HIP_LORENTZ_H
#define FDTD_HIP_LORENTZ_H

#include <stdint.h>
#include "fdtd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FDTD_LORENTZ_MAX_K 4
#define FDTD_LORENTZ_MAX_MEDIA 8

/* nmedia media (1..FDTD_LORENTZ_MAX_MEDIA) of K poles each (1..FDTD_LORENTZ_MAX_K; pad a shorter medium with zeros):
 * phi is [nmedia][K][2][2], gam and h are [nmedia][K][2].  Per component c: the box lo[c][axis] <= index < hi[c][axis] (axis
 * 0..2 = x, y, z; an empty box, hi <= lo on any axis, means the component has no dispersive edge), w[c] the weights w_e and
 * med[c] the medium ids over that box, [z][y][x] with x fastest and no padding (w[c] == 0: not dispersive; med[c] may be NULL
 * when nmedia is 1).  Every box edge must exist (index along the edge's own axis < n - 1).  The edges' vi are taken from the
 * operator, so: call after the operator is set and before the first timestep (else FDTD_E_STATE); a second call replaces the
 * set, nmedia = 0 removes it. */
int fdtd_lorentz_set(fdtd_ctx* ctx, int nmedia, int K, const float* phi, const float* gam, const float* h,
                     const int32_t lo[3][3], const int32_t hi[3][3], const float* const w[3], const uint8_t* const med[3]);

/* State of component comp's box, for tests, in the layout of fdtd_lorentz_set (the caller's box, not the widened one):
 * v_prev [box], x [K][2][box] (j_k, then u_k), vi [box] (the coefficient the correction multiplies by); any may be NULL. */
int fdtd_lorentz_get(fdtd_ctx* ctx, int comp, float* v_prev, float* x, float* vi);

#ifdef __cplusplus
}
#endif
#endif
