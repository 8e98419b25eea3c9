// farfield.hip — near-to-far-field radiation integral on the GPU (K7).
// Replaces the integral inside nf2ff.CalcNF2FF(...) (antenna_sim/solver_fdtd_openems_fixed.py:296;
// per-phi loops at solver_fdtd_openems_microstrip_3d.py:224-225, _multi_3d.py:620-621): one launch
// covers the whole theta x phi grid.  FF_DIRS directions per block, fp64 accumulation, tree reduction.
#include <math.h>

#include <cmath>

#include "fdtd_ctx.h"
#include "../../include/fdtd_hip_farfield.h"

namespace {
constexpr int FF_BLOCK = 256;
// Directions per block: every direction needs every quadrature point, so a block that serves ONE direction streams the
// whole point set (120 bytes per point) for 12 complex sums — 800x800x120 with 91 x 73 directions: 6643 x 180 MB = 1.2 TB
// through L2 / the Infinity Cache, 0.16 s, memory-bound.  FF_DIRS directions per block read each point once for all of
// them.  Per direction the summation order is unchanged (thread t takes points t, t + 256, ...; then the tree), so the
// results are the same bits as with one direction per block.
constexpr int FF_DIRS = 4;

__global__ __launch_bounds__(FF_BLOCK) void k_farfield(const int npts, const double* __restrict__ pos,
                                                       const double* __restrict__ Js, const double* __restrict__ Ms,
                                                       const double kw, const int nang, const double* __restrict__ theta,
                                                       const double* __restrict__ phi, double* __restrict__ Eth,
                                                       double* __restrict__ Eph) {
  __shared__ double red[12][FF_BLOCK];
  const int a0 = blockIdx.x * FF_DIRS;
  double rx[FF_DIRS], ry[FF_DIRS], rz[FF_DIRS];
#pragma unroll
  for (int d = 0; d < FF_DIRS; ++d) {
    const int a = min(a0 + d, nang - 1);
    double st, ct, sp, cp;
    sincos(theta[a], &st, &ct);
    sincos(phi[a], &sp, &cp);
    rx[d] = st * cp; ry[d] = st * sp; rz[d] = ct;
  }
  double acc[FF_DIRS][12];
#pragma unroll
  for (int d = 0; d < FF_DIRS; ++d)
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[d][q] = 0.0;
  for (int p = threadIdx.x; p < npts; p += FF_BLOCK) {
    const double px = pos[3 * p], py = pos[3 * p + 1], pz = pos[3 * p + 2];
    double jm[12];
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      jm[4 * n] = Js[(3 * p + n) * 2]; jm[4 * n + 1] = Js[(3 * p + n) * 2 + 1];
      jm[4 * n + 2] = Ms[(3 * p + n) * 2]; jm[4 * n + 3] = Ms[(3 * p + n) * 2 + 1];
    }
#pragma unroll
    for (int d = 0; d < FF_DIRS; ++d) {
      const double ph = kw * (rx[d] * px + ry[d] * py + rz[d] * pz);
      double ci, cr;
      sincos(ph, &ci, &cr);
#pragma unroll
      for (int n = 0; n < 3; ++n) {
        const double jr = jm[4 * n], ji = jm[4 * n + 1], mr = jm[4 * n + 2], mi = jm[4 * n + 3];
        acc[d][2 * n] += jr * cr - ji * ci;
        acc[d][2 * n + 1] += jr * ci + ji * cr;
        acc[d][6 + 2 * n] += mr * cr - mi * ci;
        acc[d][6 + 2 * n + 1] += mr * ci + mi * cr;
      }
    }
  }
#pragma unroll
  for (int d = 0; d < FF_DIRS; ++d) {
    const int a = a0 + d;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 12; ++q) red[q][threadIdx.x] = acc[d][q];
    __syncthreads();
    for (int w = FF_BLOCK / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w)
        for (int q = 0; q < 12; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0 && a < nang) {
      double st, ct, sp, cp;
      sincos(theta[a], &st, &ct);
      sincos(phi[a], &sp, &cp);
      const double eta0 = 376.730313668;
      const double fac = kw / (4.0 * M_PI);
      double Nth[2], Nph[2], Lth[2], Lph[2];
      for (int z = 0; z < 2; ++z) {
        const double Nx = red[0 + z][0], Ny = red[2 + z][0], Nz = red[4 + z][0];
        const double Lx = red[6 + z][0], Ly = red[8 + z][0], Lz = red[10 + z][0];
        Nth[z] = Nx * ct * cp + Ny * ct * sp - Nz * st;
        Nph[z] = -Nx * sp + Ny * cp;
        Lth[z] = Lx * ct * cp + Ly * ct * sp - Lz * st;
        Lph[z] = -Lx * sp + Ly * cp;
      }
      const double ar = Lph[0] + eta0 * Nth[0], ai = Lph[1] + eta0 * Nth[1];
      Eth[2 * a] = fac * ai; Eth[2 * a + 1] = -fac * ar;
      const double br = Lth[0] - eta0 * Nph[0], bi = Lth[1] - eta0 * Nph[1];
      Eph[2 * a] = -fac * bi; Eph[2 * a + 1] = fac * br;
    }
  }
}

// ---- mirror planes: the far field of a PEC / PMC symmetry half (fdtd_farfield_mirror) ---------------------------------------------
// Up to three planes (one per axis) make 2^m images of every quadrature point.  The bound above holds: a thread reads a point once
// (120 bytes) and forms its images in registers — the point set is never duplicated.  FFImages is the host's table of the images in
// counter order (bit b of the image index = reflected in plane b; image 0 is the point itself and is used as read): a position is
// fma(sp, p, off) = 2 c - p on a reflected axis, a current's term carries sj or sm = +-1 (exact).  Per direction thread t takes
// points t, t + 256, ... and per point the images in counter order, then the tree of k_farfield: with no plane the operations are
// k_farfield's, so the results are its bits.  A direction behind a half-space plane (behind[] below) gets exact zeros.
struct FFImages {
  double off[8][3], sp[8][3];   // p'_n = fma(sp_n, p_n, off_n)
  double sj[8][3], sm[8][3];    // J'_n = sj_n J_n, M'_n = sm_n M_n (+-1)
  int half_axis;                // the axis of the half-space plane, -1 without
  double half_n;                // +1 / -1: its normal n = half_n e_axis points into the simulated half
};
// r^ . n of a direction on the horizon is a rounding error of the sines and cosines away from zero (cos of the double nearest pi / 2
// is 6e-17): "behind" starts beyond that
constexpr double FF_HORIZON = -0x1p-50;

template <int M>
__global__ __launch_bounds__(FF_BLOCK) void k_farfield_mirror(const int npts, const double* __restrict__ pos,
                                                              const double* __restrict__ Js, const double* __restrict__ Ms,
                                                              const double kw, const FFImages im, const int nang,
                                                              const double* __restrict__ theta, const double* __restrict__ phi,
                                                              double* __restrict__ Eth, double* __restrict__ Eph) {
  constexpr int NIMG = 1 << M;
  __shared__ double red[12][FF_BLOCK];
  const int a0 = blockIdx.x * FF_DIRS;
  double rx[FF_DIRS], ry[FF_DIRS], rz[FF_DIRS];
  bool behind[FF_DIRS];
  bool any_front = false;
#pragma unroll
  for (int d = 0; d < FF_DIRS; ++d) {
    const int a = min(a0 + d, nang - 1);
    double st, ct, sp, cp;
    sincos(theta[a], &st, &ct);
    sincos(phi[a], &sp, &cp);
    rx[d] = st * cp; ry[d] = st * sp; rz[d] = ct;
    const double rn = im.half_axis == 0 ? rx[d] : im.half_axis == 1 ? ry[d] : rz[d];
    behind[d] = im.half_axis >= 0 && im.half_n * rn < FF_HORIZON;
    any_front = any_front || !behind[d];
  }
  double acc[FF_DIRS][12];
#pragma unroll
  for (int d = 0; d < FF_DIRS; ++d)
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[d][q] = 0.0;
  for (int p = threadIdx.x; p < npts && any_front; p += FF_BLOCK) {   // any_front is the same for the whole block
    const double px = pos[3 * p], py = pos[3 * p + 1], pz = pos[3 * p + 2];
    double jm[12];
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      jm[4 * n] = Js[(3 * p + n) * 2]; jm[4 * n + 1] = Js[(3 * p + n) * 2 + 1];
      jm[4 * n + 2] = Ms[(3 * p + n) * 2]; jm[4 * n + 3] = Ms[(3 * p + n) * 2 + 1];
    }
#pragma unroll
    for (int i = 0; i < NIMG; ++i) {
      const double qx = i ? fma(im.sp[i][0], px, im.off[i][0]) : px;
      const double qy = i ? fma(im.sp[i][1], py, im.off[i][1]) : py;
      const double qz = i ? fma(im.sp[i][2], pz, im.off[i][2]) : pz;
#pragma unroll
      for (int d = 0; d < FF_DIRS; ++d) {
        const double ph = kw * (rx[d] * qx + ry[d] * qy + rz[d] * qz);
        double ci, cr;
        sincos(ph, &ci, &cr);
#pragma unroll
        for (int n = 0; n < 3; ++n) {
          const double jr = jm[4 * n], ji = jm[4 * n + 1], mr = jm[4 * n + 2], mi = jm[4 * n + 3];
          if (i == 0) {
            acc[d][2 * n] += jr * cr - ji * ci;
            acc[d][2 * n + 1] += jr * ci + ji * cr;
            acc[d][6 + 2 * n] += mr * cr - mi * ci;
            acc[d][6 + 2 * n + 1] += mr * ci + mi * cr;
          } else {
            // the sign goes onto the finished term (s (a b - c d) = (s a) b - (s c) d in floating point too, s = +-1) and the
            // fma adds it with the one rounding of the sum above: no signed copy of the twelve currents per image is kept
            acc[d][2 * n] = fma(im.sj[i][n], jr * cr - ji * ci, acc[d][2 * n]);
            acc[d][2 * n + 1] = fma(im.sj[i][n], jr * ci + ji * cr, acc[d][2 * n + 1]);
            acc[d][6 + 2 * n] = fma(im.sm[i][n], mr * cr - mi * ci, acc[d][6 + 2 * n]);
            acc[d][6 + 2 * n + 1] = fma(im.sm[i][n], mr * ci + mi * cr, acc[d][6 + 2 * n + 1]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int d = 0; d < FF_DIRS; ++d) {
    const int a = a0 + d;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 12; ++q) red[q][threadIdx.x] = acc[d][q];
    __syncthreads();
    for (int w = FF_BLOCK / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w)
        for (int q = 0; q < 12; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0 && a < nang) {
      if (behind[d]) {
        Eth[2 * a] = 0.0; Eth[2 * a + 1] = 0.0;
        Eph[2 * a] = 0.0; Eph[2 * a + 1] = 0.0;
        continue;
      }
      double st, ct, sp, cp;
      sincos(theta[a], &st, &ct);
      sincos(phi[a], &sp, &cp);
      const double eta0 = 376.730313668;
      const double fac = kw / (4.0 * M_PI);
      double Nth[2], Nph[2], Lth[2], Lph[2];
      for (int z = 0; z < 2; ++z) {
        const double Nx = red[0 + z][0], Ny = red[2 + z][0], Nz = red[4 + z][0];
        const double Lx = red[6 + z][0], Ly = red[8 + z][0], Lz = red[10 + z][0];
        Nth[z] = Nx * ct * cp + Ny * ct * sp - Nz * st;
        Nph[z] = -Nx * sp + Ny * cp;
        Lth[z] = Lx * ct * cp + Ly * ct * sp - Lz * st;
        Lph[z] = -Lx * sp + Ly * cp;
      }
      const double ar = Lph[0] + eta0 * Nth[0], ai = Lph[1] + eta0 * Nth[1];
      Eth[2 * a] = fac * ai; Eth[2 * a + 1] = -fac * ar;
      const double br = Lth[0] - eta0 * Nph[0], bi = Lth[1] - eta0 * Nph[1];
      Eph[2 * a] = -fac * bi; Eph[2 * a + 1] = fac * br;
    }
  }
}
}  // namespace

extern "C" int fdtd_farfield(int device, int npts, const double* pos, const double* Js, const double* Ms, double kw,
                             int nang, const double* theta, const double* phi, double* Eth, double* Eph) {
  if (npts < 0 || nang < 0 || !pos || !Js || !Ms || !theta || !phi || !Eth || !Eph)
    return fdtd_fail(nullptr, FDTD_E_ARG, "bad farfield argument");
  if (nang == 0) return FDTD_OK;
  HIPCK(nullptr, hipSetDevice(device));
  double *d_pos = nullptr, *d_J = nullptr, *d_M = nullptr, *d_th = nullptr, *d_ph = nullptr, *d_eth = nullptr, *d_eph = nullptr;
  const size_t np = (size_t)(npts > 0 ? npts : 1);
  int rc = FDTD_OK;
#define FF(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess && rc == FDTD_OK) rc = fdtd_fail(nullptr, FDTD_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); } while (0)
  FF(hipMalloc(&d_pos, np * 3 * sizeof(double)));
  FF(hipMalloc(&d_J, np * 6 * sizeof(double)));
  FF(hipMalloc(&d_M, np * 6 * sizeof(double)));
  FF(hipMalloc(&d_th, nang * sizeof(double)));
  FF(hipMalloc(&d_ph, nang * sizeof(double)));
  FF(hipMalloc(&d_eth, nang * 2 * sizeof(double)));
  FF(hipMalloc(&d_eph, nang * 2 * sizeof(double)));
  if (rc == FDTD_OK) {
    if (npts > 0) {
      FF(hipMemcpy(d_pos, pos, (size_t)npts * 3 * sizeof(double), hipMemcpyHostToDevice));
      FF(hipMemcpy(d_J, Js, (size_t)npts * 6 * sizeof(double), hipMemcpyHostToDevice));
      FF(hipMemcpy(d_M, Ms, (size_t)npts * 6 * sizeof(double), hipMemcpyHostToDevice));
    }
    FF(hipMemcpy(d_th, theta, nang * sizeof(double), hipMemcpyHostToDevice));
    FF(hipMemcpy(d_ph, phi, nang * sizeof(double), hipMemcpyHostToDevice));
    if (rc == FDTD_OK) {
      hipLaunchKernelGGL(k_farfield, dim3((nang + FF_DIRS - 1) / FF_DIRS), dim3(FF_BLOCK), 0, 0, npts, d_pos, d_J, d_M, kw, nang, d_th, d_ph, d_eth, d_eph);
      FF(hipGetLastError());
      FF(hipDeviceSynchronize());
      FF(hipMemcpy(Eth, d_eth, nang * 2 * sizeof(double), hipMemcpyDeviceToHost));
      FF(hipMemcpy(Eph, d_eph, nang * 2 * sizeof(double), hipMemcpyDeviceToHost));
    }
  }
#undef FF
  hipFree(d_pos); hipFree(d_J); hipFree(d_M); hipFree(d_th); hipFree(d_ph); hipFree(d_eth); hipFree(d_eph);
  return rc;
}

extern "C" int fdtd_farfield_mirror(int device, int npts, const double* pos, const double* Js, const double* Ms, double kw, int nmirror,
                                    const int* mirror_axis, const int* mirror_type, const double* mirror_coord, int half_space_plane,
                                    int nang, const double* theta, const double* phi, double* Eth, double* Eph) {
  if (npts < 0 || nang < 0 || !pos || !Js || !Ms || !theta || !phi || !Eth || !Eph)
    return fdtd_fail(nullptr, FDTD_E_ARG, "bad farfield argument");
  if (nmirror < 0 || nmirror > 3 || (nmirror > 0 && (!mirror_axis || !mirror_type || !mirror_coord)))
    return fdtd_fail(nullptr, FDTD_E_ARG, "farfield: 0 to 3 mirror planes, each with axis, type and coordinate");
  for (int b = 0; b < nmirror; ++b) {
    if (mirror_axis[b] < 0 || mirror_axis[b] > 2) return fdtd_fail(nullptr, FDTD_E_ARG, "farfield: mirror plane %d has axis %d (0, 1 or 2)", b, mirror_axis[b]);
    if (mirror_type[b] != FDTD_MIRROR_PEC && mirror_type[b] != FDTD_MIRROR_PMC)
      return fdtd_fail(nullptr, FDTD_E_ARG, "farfield: mirror plane %d has type %d (1 = PEC, 2 = PMC)", b, mirror_type[b]);
    if (!std::isfinite(mirror_coord[b])) return fdtd_fail(nullptr, FDTD_E_ARG, "farfield: mirror plane %d has no finite coordinate", b);
    for (int q = 0; q < b; ++q)
      if (mirror_axis[q] == mirror_axis[b]) return fdtd_fail(nullptr, FDTD_E_ARG, "farfield: two mirror planes on axis %d", mirror_axis[b]);
  }
  if (half_space_plane < -1 || half_space_plane >= nmirror)
    return fdtd_fail(nullptr, FDTD_E_ARG, "farfield: half-space plane %d of %d mirror planes", half_space_plane, nmirror);
  if (half_space_plane >= 0 && mirror_type[half_space_plane] != FDTD_MIRROR_PEC)
    return fdtd_fail(nullptr, FDTD_E_ARG, "farfield: the half-space plane must be a PEC plane");
  FFImages im;
  for (int i = 0; i < 8; ++i)
    for (int n = 0; n < 3; ++n) {
      im.off[i][n] = 0.0; im.sp[i][n] = 1.0; im.sj[i][n] = 1.0; im.sm[i][n] = 1.0;
    }
  for (int i = 0; i < (1 << nmirror); ++i)
    for (int b = 0; b < nmirror; ++b)
      if (i >> b & 1) {
        const int a = mirror_axis[b];
        const double s = mirror_type[b] == FDTD_MIRROR_PEC ? 1.0 : -1.0;     // PEC: J tangential -, J normal +; M the opposite; PMC the dual
        for (int n = 0; n < 3; ++n) {
          im.sj[i][n] *= n == a ? s : -s;
          im.sm[i][n] *= n == a ? -s : s;
        }
        im.off[i][a] = 2.0 * mirror_coord[b];       // one plane per axis: set once
        im.sp[i][a] = -1.0;
      }
  im.half_axis = -1; im.half_n = 1.0;
  if (half_space_plane >= 0) {
    // the simulated half is where the points are: the first point off the plane tells the side, and all must share it
    const int a = mirror_axis[half_space_plane];
    const double c = mirror_coord[half_space_plane];
    int side = 0;
    for (int p = 0; p < npts; ++p) {
      const double x = pos[3 * (size_t)p + a];
      const int s = x > c ? 1 : x < c ? -1 : 0;
      if (s && side && s != side) return fdtd_fail(nullptr, FDTD_E_ARG, "farfield: points on both sides of the half-space plane");
      if (s) side = s;
    }
    im.half_axis = a; im.half_n = side < 0 ? -1.0 : 1.0;
  }
  if (nang == 0) return FDTD_OK;
  HIPCK(nullptr, hipSetDevice(device));
  double *d_pos = nullptr, *d_J = nullptr, *d_M = nullptr, *d_th = nullptr, *d_ph = nullptr, *d_eth = nullptr, *d_eph = nullptr;
  const size_t np = (size_t)(npts > 0 ? npts : 1);
  int rc = FDTD_OK;
#define FF(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess && rc == FDTD_OK) rc = fdtd_fail(nullptr, FDTD_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); } while (0)
  FF(hipMalloc(&d_pos, np * 3 * sizeof(double)));
  FF(hipMalloc(&d_J, np * 6 * sizeof(double)));
  FF(hipMalloc(&d_M, np * 6 * sizeof(double)));
  FF(hipMalloc(&d_th, nang * sizeof(double)));
  FF(hipMalloc(&d_ph, nang * sizeof(double)));
  FF(hipMalloc(&d_eth, nang * 2 * sizeof(double)));
  FF(hipMalloc(&d_eph, nang * 2 * sizeof(double)));
  if (rc == FDTD_OK) {
    if (npts > 0) {
      FF(hipMemcpy(d_pos, pos, (size_t)npts * 3 * sizeof(double), hipMemcpyHostToDevice));
      FF(hipMemcpy(d_J, Js, (size_t)npts * 6 * sizeof(double), hipMemcpyHostToDevice));
      FF(hipMemcpy(d_M, Ms, (size_t)npts * 6 * sizeof(double), hipMemcpyHostToDevice));
    }
    FF(hipMemcpy(d_th, theta, nang * sizeof(double), hipMemcpyHostToDevice));
    FF(hipMemcpy(d_ph, phi, nang * sizeof(double), hipMemcpyHostToDevice));
    if (rc == FDTD_OK) {
      const dim3 grid((nang + FF_DIRS - 1) / FF_DIRS), block(FF_BLOCK);
      switch (nmirror) {   // the plane count is a template parameter: the image loop unrolls
        case 0: hipLaunchKernelGGL(k_farfield_mirror<0>, grid, block, 0, 0, npts, d_pos, d_J, d_M, kw, im, nang, d_th, d_ph, d_eth, d_eph); break;
        case 1: hipLaunchKernelGGL(k_farfield_mirror<1>, grid, block, 0, 0, npts, d_pos, d_J, d_M, kw, im, nang, d_th, d_ph, d_eth, d_eph); break;
        case 2: hipLaunchKernelGGL(k_farfield_mirror<2>, grid, block, 0, 0, npts, d_pos, d_J, d_M, kw, im, nang, d_th, d_ph, d_eth, d_eph); break;
        default: hipLaunchKernelGGL(k_farfield_mirror<3>, grid, block, 0, 0, npts, d_pos, d_J, d_M, kw, im, nang, d_th, d_ph, d_eth, d_eph); break;
      }
      FF(hipGetLastError());
      FF(hipDeviceSynchronize());
      FF(hipMemcpy(Eth, d_eth, nang * 2 * sizeof(double), hipMemcpyDeviceToHost));
      FF(hipMemcpy(Eph, d_eph, nang * 2 * sizeof(double), hipMemcpyDeviceToHost));
    }
  }
#undef FF
  hipFree(d_pos); hipFree(d_J); hipFree(d_M); hipFree(d_th); hipFree(d_ph); hipFree(d_eth); hipFree(d_eph);
  return rc;
}
