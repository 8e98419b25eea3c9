/* fdtd_hip_sar.h — specific absorption rate of a volume box on the device: local SAR from the frequency-domain edge voltages, and
 * the 1 g / 10 g mass average (a centred cube grown around every voxel until it holds the mass).  Exported by libfdtd_hip.so only;
 * not part of fdtd_hip.h nor of FDTD_ABI_VERSION (as the other feature headers).  Both calls are stateless, take host pointers and
 * touch no context: they run after the time stepping.
 *
 * The numpy module sar.py is the specification and spells the arithmetic; its text is not repeated here.  The box has ncx x ncy x ncz
 * cells, per-cell arrays are double [ncz][ncy][ncx], dx / dy / dz the cell sizes in metres.
 *
 * fdtd_sar_local gives sar.local_spec bit for bit: float64, + - * / in the association of sar.py, the library compiled with
 * -ffp-contract=off.  fdtd_sar_average gives sar.average_spec to rounding: its sums run in another order (per lane along x, lanes
 * over the (y, z) columns of the cube, a fixed butterfly over the 64 lanes), always the same one — two calls give identical bits.
 */
#ifndef FDTD_HIP_SAR_H
#define FDTD_HIP_SAR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { FDTD_SAR_IEEE = 0, FDTD_SAR_SIMPLE = 1 };
/* status bytes of fdtd_sar_average */
enum { FDTD_SAR_BACKGROUND = -1, FDTD_SAR_VALID = 0, FDTD_SAR_USED = 1, FDTD_SAR_NO_CUBE = 2, FDTD_SAR_TOO_SMALL = 3 };

/* Vx, Vy, Vz: the edge voltages on the node box, double [ncz+1][ncy+1][ncx+1][2] (re, im); sigma [S/m] and rho [kg/m^3, 0:
 * background] per cell.  p_out [W/m^3] and sar_out [W/kg] per cell.  Returns FDTD_OK or a negative FDTD_E_* code (message:
 * fdtd_last_error(NULL)). */
int fdtd_sar_local(int device, int ncx, int ncy, int ncz, const double* dx, const double* dy, const double* dz, const double* Vx,
                   const double* Vy, const double* Vz, const double* sigma, const double* rho, double* p_out, double* sar_out);

/* rho, p per cell (finite, >= 0); mass [kg] > 0; method FDTD_SAR_IEEE or FDTD_SAR_SIMPLE.  sar_avg, half_side: double per cell (NaN
 * where sar.py says so); status: int8 per cell; counts: int64 [4], the voxels of status 0..3. */
int fdtd_sar_average(int device, int ncx, int ncy, int ncz, const double* dx, const double* dy, const double* dz, const double* rho,
                     const double* p, double mass, int method, double* sar_avg, double* half_side, int8_t* status, int64_t* counts);

#ifdef __cplusplus
}
#endif
#endif
