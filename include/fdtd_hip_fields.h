/* fdtd_hip_fields.h — field dumps on the device: the recorded edge voltages or face currents of a volume box turned into E, H, J or
 * rot-H on a point lattice (raw, node-interpolated or cell-interpolated, sub-sampled).  Exported by libfdtd_hip.so only; not part of
 * fdtd_hip.h nor of FDTD_ABI_VERSION (as the other feature headers).  The call is stateless, takes host pointers and touches no
 * context: it runs after the time stepping.
 *
 * The numpy module fields.py is the specification and spells every rule and the arithmetic; its text is not repeated here.
 * fdtd_field_interp gives fields.interp_spec bit for bit: float64, + - * / in the association of fields.py, the library compiled
 * with -ffp-contract=off.
 */
#ifndef FDTD_HIP_FIELDS_H
#define FDTD_HIP_FIELDS_H

#ifdef __cplusplus
extern "C" {
#endif

enum { FDTD_FIELD_E = 0, FDTD_FIELD_H = 1, FDTD_FIELD_J = 2, FDTD_FIELD_ROTH = 3 };
enum { FDTD_FIELD_RAW = 0, FDTD_FIELD_NODE = 1, FDTD_FIELD_CELL = 2 };

/* n: the grid's node counts; x, y, z: its node lines (n[0], n[1], n[2] doubles, strictly increasing); lo, hi: the dump box in nodes;
 * sub: the sub-sampling strides (>= 1).  parts: 1 for real samples, 2 for interleaved complex spectra (re, im).
 * rec0..rec2: the recorded arrays of components x, y, z over the region max(lo - 1, 0)..hi, double [rnz][rny][rnx][parts] — edge
 * voltages for FDTD_FIELD_E and _J, face currents for _H and _ROTH.  kap0..kap2: the edge conductivities over the region, double
 * [rnz][rny][rnx] (FDTD_FIELD_J; NULL otherwise).  out: double [3][onz][ony][onx][parts], on = (extent - 1) / sub + 1 points per
 * axis with extent = hi - lo + 1 nodes, or hi - lo cells for FDTD_FIELD_CELL (which needs hi > lo on every axis).
 * Returns FDTD_OK or a negative FDTD_E_* code (message: fdtd_last_error(NULL)). */
int fdtd_field_interp(int device, int kind, int mode, int parts, const int* n, const int* lo, const int* hi, const int* sub,
                      const double* x, const double* y, const double* z, const double* rec0, const double* rec1, const double* rec2,
                      const double* kap0, const double* kap1, const double* kap2, double* out);

#ifdef __cplusplus
}
#endif
#endif
