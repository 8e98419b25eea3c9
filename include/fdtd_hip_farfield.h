/* fdtd_hip_farfield.h — the radiation integral of fdtd_farfield (fdtd_hip.h) over a PEC / PMC symmetry half and its mirror images.
 * Exported by libfdtd_hip.so only; not part of fdtd_hip.h nor of FDTD_ABI_VERSION (as the other feature headers).  The call is
 * stateless, takes host pointers and touches no context: it runs after the time stepping.  The numpy statement is
 * nf2ff.farfield_mirror_spec.
 */
#ifndef FDTD_HIP_FARFIELD_H
#define FDTD_HIP_FARFIELD_H

#ifdef __cplusplus
extern "C" {
#endif

/* pos, Js, Ms, k_wave, theta, phi, Eth, Eph: as fdtd_farfield takes them.  nmirror = 0..3 planes, at most one per
 * axis: plane b is normal to mirror_axis[b] (0 x, 1 y, 2 z) at mirror_coord[b] (metres, relative to the phase
 * centre like pos) and of mirror_type[b] (upstream's numbers).  Every point has 2^nmirror images; bit b of the
 * image index = reflected in plane b, image 0 is the point itself.  Reflected in a plane normal to a:
 *   position  r'_a = 2 c - r_a, the other coordinates unchanged
 *   PEC:  J tangential x(-1), J_a x(+1);  M tangential x(+1), M_a x(-1)        PMC: the dual (all four signs flipped)
 * Several planes compose, the signs multiply.  The images are formed in registers: the point set is read once per
 * block of directions, as by fdtd_farfield, and with nmirror = 0 the result is bit for bit fdtd_farfield's.
 * half_space_plane = b (-1: none) names one PEC plane as an infinite ground: directions with r^ . n < 0 get exact
 * zeros, n being the plane's normal into the half where the points lie (points on both sides: FDTD_E_ARG); a
 * direction on the horizon counts as in front (r^ . n >= -2^-50: the rounding of sin and cos of a double angle). */
#define FDTD_MIRROR_PEC 1
#define FDTD_MIRROR_PMC 2
int fdtd_farfield_mirror(int device, int npts, const double* pos, const double* Js, const double* Ms,
                         double k_wave, int nmirror, const int* mirror_axis, const int* mirror_type,
                         const double* mirror_coord, int half_space_plane, int nang, const double* theta,
                         const double* phi, double* Eth, double* Eph);

#ifdef __cplusplus
}
#endif
#endif
