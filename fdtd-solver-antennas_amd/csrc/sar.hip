// sar.hip — local and mass-averaged SAR of a volume box (include/fdtd_hip_sar.h; sar.py is the specification).  Stateless: host
// pointers in, host pointers out, no context, none of the step schedules.
//
// k_sar_local: one thread per cell, float64 in the association sar.py spells (-ffp-contract=off keeps the compiler from fusing), so
// p and sar_local have the specification's bits.
//
// k_sar_cube: one wave per voxel.  A cube of half-side h about the voxel's centre overlaps the cells ia..ib x ja..jb x ka..kb; the
// lanes take the (j, k) columns of that range, 64 at a time, and run serially along x.  The x weights of up to 64 cells sit one per
// lane in a register and reach the other lanes by readlane (the x index is wave-uniform); the y and z weights are recomputed per
// column.  No LDS, no barrier: the four waves of a block work on four voxels and never meet.  The lane totals are added by an xor
// butterfly over the 64 lanes, the same order in every call, and every lane ends with the same bits, so the 48 bisection branches are
// wave-uniform.  m, P and Vbg at h* come out of one pass.
//
// k_sar_second: the "ieee" second pass as a gather, one thread per voxel: a status-1 voxel looks at the voxels whose centres lie
// within the largest valid half-side of its own (index ranges per axis) and takes the largest sar_avg of the status-0 cubes that hold
// its centre.  It writes only its own entries and reads only status-0 ones, which nobody writes: in place, no atomics.
#include <math.h>
#include <stdint.h>

#include <vector>

#include "fdtd_ctx.h"
#include "../../include/fdtd_hip_sar.h"

namespace {
constexpr int SAR_BLOCK = 256, SAR_WAVES = SAR_BLOCK / 64;
constexpr int SAR_NBISECT = 48;          // sar.N_BISECT
constexpr double SAR_BG_FRACTION = 0.1;  // sar.BG_FRACTION

struct LocalArgs {
  int ncx, ncy, ncz;
  const double *dx, *dy, *dz;
  const double* V[3];     // [ncz+1][ncy+1][ncx+1][2]
  const double *sigma, *rho;
  double *p, *sar;
};

// q_c of sar.py for the four edges at flat node offsets o0..o3
__device__ __forceinline__ double centre_sq(const double* __restrict__ V, size_t o0, size_t o1, size_t o2, size_t o3, double d) {
  const double sr = (V[2 * o0] + V[2 * o1]) + (V[2 * o2] + V[2 * o3]);
  const double si = (V[2 * o0 + 1] + V[2 * o1 + 1]) + (V[2 * o2 + 1] + V[2 * o3 + 1]);
  const double er = (0.25 * sr) / d, ei = (0.25 * si) / d;
  return er * er + ei * ei;
}

__global__ __launch_bounds__(SAR_BLOCK) void k_sar_local(const LocalArgs a) {
  const long long q = (long long)blockIdx.x * SAR_BLOCK + threadIdx.x;
  const long long ncell = (long long)a.ncx * a.ncy * a.ncz;
  if (q >= ncell) return;
  const int i = (int)(q % a.ncx), j = (int)((q / a.ncx) % a.ncy), k = (int)(q / ((long long)a.ncx * a.ncy));
  const size_t sx = 1, sy = (size_t)a.ncx + 1, sz = sy * ((size_t)a.ncy + 1);
  const size_t n = (size_t)k * sz + (size_t)j * sy + (size_t)i;
  const double qx = centre_sq(a.V[0], n, n + sy, n + sz, n + sy + sz, a.dx[i]);
  const double qy = centre_sq(a.V[1], n, n + sx, n + sz, n + sx + sz, a.dy[j]);
  const double qz = centre_sq(a.V[2], n, n + sx, n + sy, n + sx + sy, a.dz[k]);
  const double p = (0.5 * a.sigma[q]) * ((qx + qy) + qz);
  const double rho = a.rho[q];
  a.p[q] = p;
  a.sar[q] = rho > 0.0 ? p / rho : 0.0;
}

struct CubeArgs {
  int ncx, ncy, ncz;
  const double *ex, *ey, *ez;   // node coordinates, ncx + 1, ncy + 1, ncz + 1
  const double *rho, *p;
  double mass;
  int method;
  long long nvox;
  double *sar, *half;
  int8_t* status;
};

// the cells a..b of one axis (n cells, node coordinates e) that [lo, hi] can overlap: sar.overlap
__device__ __forceinline__ void axis_range(const double* __restrict__ e, int n, double lo, double hi, int& a, int& b) {
  int l = 0, r = n + 1;
  while (l < r) { const int m = (l + r) >> 1; if (e[m] <= lo) l = m + 1; else r = m; }
  a = min(max(l - 1, 0), n - 1);
  l = 0; r = n + 1;
  while (l < r) { const int m = (l + r) >> 1; if (e[m] < hi) l = m + 1; else r = m; }
  b = min(max(l - 1, a), n - 1);
}

__device__ __forceinline__ double axis_weight(const double* __restrict__ e, int i, double lo, double hi) {
  return fmax(0.0, fmin(e[i + 1], hi) - fmax(e[i], lo));
}

// v of lane `l` (wave-uniform) in every lane
__device__ __forceinline__ double lane_value(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s, 64);
  return v;
}

// m(h) and, FULL, P(h) and Vbg(h) about the centre (cx, cy, cz); the whole wave calls it and every lane gets the sums
template <bool FULL>
__device__ __forceinline__ void cube_sums(const CubeArgs& a, const int lane, const double cx, const double cy, const double cz,
                                          const double h, double& m, double& P, double& bg) {
  const double xl = cx - h, xh = cx + h, yl = cy - h, yh = cy + h, zl = cz - h, zh = cz + h;
  int ia, ib, ja, jb, ka, kb;
  axis_range(a.ex, a.ncx, xl, xh, ia, ib);
  axis_range(a.ey, a.ncy, yl, yh, ja, jb);
  axis_range(a.ez, a.ncz, zl, zh, ka, kb);
  const int nj = jb - ja + 1, ncol = nj * (kb - ka + 1);
  double tm = 0.0, tp = 0.0, tb = 0.0;
  for (int i0 = ia; i0 <= ib; i0 += 64) {
    const int n = min(64, ib - i0 + 1);
    const double wxr = lane < n ? axis_weight(a.ex, i0 + lane, xl, xh) : 0.0;
    for (int c0 = 0; c0 < ncol; c0 += 64) {
      const bool on = c0 + lane < ncol;
      const int col = on ? c0 + lane : 0;                          // an idle lane reads column 0 with weight 0
      const int jj = ja + col % nj, kk = ka + col / nj;
      const double wyz = on ? axis_weight(a.ey, jj, yl, yh) * axis_weight(a.ez, kk, zl, zh) : 0.0;
      const size_t base = ((size_t)kk * (size_t)a.ncy + (size_t)jj) * (size_t)a.ncx + (size_t)i0;
      double am = 0.0, ap = 0.0, ab = 0.0;
      for (int t = 0; t < n; ++t) {
        const double w = lane_value(wxr, t);
        const double r = a.rho[base + t];
        am += w * r;
        if (FULL) {
          ap += w * a.p[base + t];
          ab += r == 0.0 ? w : 0.0;
        }
      }
      tm += wyz * am;
      if (FULL) { tp += wyz * ap; tb += wyz * ab; }
    }
  }
  m = wave_sum(tm);
  if (FULL) { P = wave_sum(tp); bg = wave_sum(tb); }
}

__global__ __launch_bounds__(SAR_BLOCK) void k_sar_cube(const CubeArgs a) {
  const int lane = threadIdx.x & 63;
  const long long vox = (long long)blockIdx.x * SAR_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (vox >= a.nvox) return;                                       // the whole wave
  const int i = (int)(vox % a.ncx), j = (int)((vox / a.ncx) % a.ncy), k = (int)(vox / ((long long)a.ncx * a.ncy));
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double sar = 0.0, half = nan;
  int st = FDTD_SAR_BACKGROUND;
  if (a.rho[vox] > 0.0) {                                          // wave-uniform
    const double cx = 0.5 * (a.ex[i] + a.ex[i + 1]), cy = 0.5 * (a.ey[j] + a.ey[j + 1]), cz = 0.5 * (a.ez[k] + a.ez[k + 1]);
    const double hmax = fmin(fmin(fmin(cx, a.ex[a.ncx] - cx), fmin(cy, a.ey[a.ncy] - cy)), fmin(cz, a.ez[a.ncz] - cz));
    double m, P = 0.0, bg = 0.0;
    cube_sums<false>(a, lane, cx, cy, cz, hmax, m, P, bg);
    if (m < a.mass) {
      st = FDTD_SAR_TOO_SMALL;
      sar = nan;
    } else {
      double lo = 0.0, hi = hmax;
      for (int it = 0; it < SAR_NBISECT; ++it) {
        const double mid = 0.5 * (lo + hi);
        cube_sums<false>(a, lane, cx, cy, cz, mid, m, P, bg);
        if (m >= a.mass) hi = mid; else lo = mid;
      }
      cube_sums<true>(a, lane, cx, cy, cz, hi, m, P, bg);
      sar = P / m;
      half = hi;
      const double side = 2.0 * hi;
      const double lim = SAR_BG_FRACTION * ((side * side) * side);
      st = (a.method == FDTD_SAR_IEEE && !(bg <= lim)) ? FDTD_SAR_USED : FDTD_SAR_VALID;
    }
  }
  if (lane == 0) {
    a.sar[vox] = sar;
    a.half[vox] = half;
    a.status[vox] = (int8_t)st;
  }
}

struct SecondArgs {
  int ncx, ncy, ncz;
  const double *cx, *cy, *cz;   // cell centres
  double hmax;                  // the largest half-side of a status-0 voxel
  const double* half;
  double* sar;
  int8_t* status;
};

// cells a..b of one axis whose centres lie within h of centre i (a superset is enough: every candidate is tested)
__device__ __forceinline__ void centre_range(const double* __restrict__ c, int n, int i, double h, int& a, int& b) {
  a = i; b = i;
  while (a > 0 && c[i] - c[a - 1] <= h) --a;
  while (b < n - 1 && c[b + 1] - c[i] <= h) ++b;
}

__global__ __launch_bounds__(SAR_BLOCK) void k_sar_second(const SecondArgs a) {
  const long long q = (long long)blockIdx.x * SAR_BLOCK + threadIdx.x;
  const long long ncell = (long long)a.ncx * a.ncy * a.ncz;
  if (q >= ncell || a.status[q] != FDTD_SAR_USED) return;
  const int i = (int)(q % a.ncx), j = (int)((q / a.ncx) % a.ncy), k = (int)(q / ((long long)a.ncx * a.ncy));
  int ia, ib, ja, jb, ka, kb;
  centre_range(a.cx, a.ncx, i, a.hmax, ia, ib);
  centre_range(a.cy, a.ncy, j, a.hmax, ja, jb);
  centre_range(a.cz, a.ncz, k, a.hmax, ka, kb);
  const double x = a.cx[i], y = a.cy[j], z = a.cz[k];
  double best = -1.0;                                              // sar_avg >= 0
  for (int kk = ka; kk <= kb; ++kk)
    for (int jj = ja; jj <= jb; ++jj) {
      const size_t row = ((size_t)kk * (size_t)a.ncy + (size_t)jj) * (size_t)a.ncx;
      const double dy = fabs(y - a.cy[jj]), dz = fabs(z - a.cz[kk]);
      for (int ii = ia; ii <= ib; ++ii) {
        if (a.status[row + ii] != FDTD_SAR_VALID) continue;
        const double h0 = a.half[row + ii];
        if (fabs(x - a.cx[ii]) <= h0 && dy <= h0 && dz <= h0) best = fmax(best, a.sar[row + ii]);
      }
    }
  if (best >= 0.0) {
    a.sar[q] = best;
  } else {
    a.sar[q] = __longlong_as_double(0x7ff8000000000000LL);
    a.status[q] = FDTD_SAR_NO_CUBE;
  }
}

bool sizes_ok(int n, const double* d) {
  for (int q = 0; q < n; ++q)
    if (!(d[q] > 0.0) || !isfinite(d[q])) return false;
  return true;
}
bool cells_ok(size_t n, const double* v) {
  for (size_t q = 0; q < n; ++q)
    if (!(v[q] >= 0.0) || !isfinite(v[q])) return false;
  return true;
}
}  // namespace

#define SX(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess && rc == FDTD_OK) rc = fdtd_fail(nullptr, e_ == hipErrorOutOfMemory ? FDTD_E_NOMEM : FDTD_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); } while (0)

extern "C" int fdtd_sar_local(int device, int ncx, int ncy, int ncz, const double* dx, const double* dy, const double* dz,
                              const double* Vx, const double* Vy, const double* Vz, const double* sigma, const double* rho,
                              double* p_out, double* sar_out) {
  if (ncx < 1 || ncy < 1 || ncz < 1 || !dx || !dy || !dz || !Vx || !Vy || !Vz || !sigma || !rho || !p_out || !sar_out)
    return fdtd_fail(nullptr, FDTD_E_ARG, "bad sar_local argument");
  const long long ncell = (long long)ncx * ncy * ncz, nnode = (long long)(ncx + 1) * (ncy + 1) * (ncz + 1);
  if (nnode >= (1LL << 31)) return fdtd_fail(nullptr, FDTD_E_ARG, "sar_local: the box has %lld nodes, at most 2^31 - 1", nnode);
  if (!sizes_ok(ncx, dx) || !sizes_ok(ncy, dy) || !sizes_ok(ncz, dz))
    return fdtd_fail(nullptr, FDTD_E_ARG, "sar_local: cell sizes must be finite and > 0");
  int rc = FDTD_OK;
  HIPCK(nullptr, hipSetDevice(device));
  double *d_d = nullptr, *d_V[3] = {nullptr, nullptr, nullptr}, *d_cell = nullptr;   // d_cell: sigma, rho, p, sar
  const size_t nd = (size_t)ncx + ncy + ncz, vbytes = (size_t)nnode * 2 * sizeof(double), cbytes = (size_t)ncell * sizeof(double);
  SX(hipMalloc(&d_d, nd * sizeof(double)));
  for (int c = 0; c < 3; ++c) SX(hipMalloc(&d_V[c], vbytes));
  SX(hipMalloc(&d_cell, 4 * cbytes));
  if (rc == FDTD_OK) {
    SX(hipMemcpy(d_d, dx, (size_t)ncx * sizeof(double), hipMemcpyHostToDevice));
    SX(hipMemcpy(d_d + ncx, dy, (size_t)ncy * sizeof(double), hipMemcpyHostToDevice));
    SX(hipMemcpy(d_d + ncx + ncy, dz, (size_t)ncz * sizeof(double), hipMemcpyHostToDevice));
    const double* V[3] = {Vx, Vy, Vz};
    for (int c = 0; c < 3; ++c) SX(hipMemcpy(d_V[c], V[c], vbytes, hipMemcpyHostToDevice));
    SX(hipMemcpy(d_cell, sigma, cbytes, hipMemcpyHostToDevice));
    SX(hipMemcpy(d_cell + ncell, rho, cbytes, hipMemcpyHostToDevice));
  }
  if (rc == FDTD_OK) {
    LocalArgs a{ncx, ncy, ncz, d_d, d_d + ncx, d_d + ncx + ncy, {d_V[0], d_V[1], d_V[2]}, d_cell, d_cell + ncell,
                d_cell + 2 * ncell, d_cell + 3 * ncell};
    hipLaunchKernelGGL(k_sar_local, dim3((unsigned)((ncell + SAR_BLOCK - 1) / SAR_BLOCK)), dim3(SAR_BLOCK), 0, 0, a);
    SX(hipGetLastError());
    SX(hipDeviceSynchronize());
    if (rc == FDTD_OK) SX(hipMemcpy(p_out, d_cell + 2 * ncell, cbytes, hipMemcpyDeviceToHost));
    if (rc == FDTD_OK) SX(hipMemcpy(sar_out, d_cell + 3 * ncell, cbytes, hipMemcpyDeviceToHost));
  }
  hipFree(d_d); hipFree(d_V[0]); hipFree(d_V[1]); hipFree(d_V[2]); hipFree(d_cell);
  return rc;
}

extern "C" int fdtd_sar_average(int device, int ncx, int ncy, int ncz, const double* dx, const double* dy, const double* dz,
                                const double* rho, const double* p, double mass, int method, double* sar_avg, double* half_side,
                                int8_t* status, int64_t* counts) {
  if (ncx < 1 || ncy < 1 || ncz < 1 || !dx || !dy || !dz || !rho || !p || !sar_avg || !half_side || !status || !counts ||
      !(mass > 0.0) || !isfinite(mass) || (method != FDTD_SAR_IEEE && method != FDTD_SAR_SIMPLE))
    return fdtd_fail(nullptr, FDTD_E_ARG, "bad sar_average argument");
  const long long ncell = (long long)ncx * ncy * ncz;
  if (ncell >= (1LL << 31)) return fdtd_fail(nullptr, FDTD_E_ARG, "sar_average: the box has %lld cells, at most 2^31 - 1", ncell);
  if (!sizes_ok(ncx, dx) || !sizes_ok(ncy, dy) || !sizes_ok(ncz, dz))
    return fdtd_fail(nullptr, FDTD_E_ARG, "sar_average: cell sizes must be finite and > 0");
  if (!cells_ok((size_t)ncell, rho) || !cells_ok((size_t)ncell, p))
    return fdtd_fail(nullptr, FDTD_E_ARG, "sar_average: rho and p must be finite and >= 0");
  // node coordinates (summed in order, sar.node_lines) and cell centres: [ex ey ez | cx cy cz]
  const int nn[3] = {ncx, ncy, ncz};
  const double* dd[3] = {dx, dy, dz};
  const size_t nd = (size_t)ncx + ncy + ncz;
  std::vector<double> lines, half_h;
  std::vector<int8_t> st_h;
  try {
    lines.resize(2 * nd + 3);
    half_h.resize((size_t)ncell);
    st_h.resize((size_t)ncell);
  } catch (...) {
    return fdtd_fail(nullptr, FDTD_E_NOMEM, "sar_average: no host memory for %lld cells", ncell);
  }
  size_t eo[3], co[3];
  for (size_t a = 0, e = 0, c = nd + 3; a < 3; e += nn[a] + 1, c += nn[a], ++a) {
    eo[a] = e; co[a] = c;
    lines[e] = 0.0;
    for (int q = 0; q < nn[a]; ++q) lines[e + q + 1] = lines[e + q] + dd[a][q];
    for (int q = 0; q < nn[a]; ++q) lines[c + q] = 0.5 * (lines[e + q] + lines[e + q + 1]);
  }
  int rc = FDTD_OK;
  HIPCK(nullptr, hipSetDevice(device));
  double *d_lines = nullptr, *d_cell = nullptr;                     // d_cell: rho, p, sar, half
  int8_t* d_st = nullptr;
  const size_t cbytes = (size_t)ncell * sizeof(double);
  SX(hipMalloc(&d_lines, lines.size() * sizeof(double)));
  SX(hipMalloc(&d_cell, 4 * cbytes));
  SX(hipMalloc(&d_st, (size_t)ncell));
  if (rc == FDTD_OK) {
    SX(hipMemcpy(d_lines, lines.data(), lines.size() * sizeof(double), hipMemcpyHostToDevice));
    SX(hipMemcpy(d_cell, rho, cbytes, hipMemcpyHostToDevice));
    SX(hipMemcpy(d_cell + ncell, p, cbytes, hipMemcpyHostToDevice));
  }
  if (rc == FDTD_OK) {
    CubeArgs a{ncx, ncy, ncz, d_lines + eo[0], d_lines + eo[1], d_lines + eo[2], d_cell, d_cell + ncell, mass, method, ncell,
               d_cell + 2 * ncell, d_cell + 3 * ncell, d_st};
    hipLaunchKernelGGL(k_sar_cube, dim3((unsigned)((ncell + SAR_WAVES - 1) / SAR_WAVES)), dim3(SAR_BLOCK), 0, 0, a);
    SX(hipGetLastError());
    SX(hipDeviceSynchronize());
    if (rc == FDTD_OK) SX(hipMemcpy(half_h.data(), d_cell + 3 * ncell, cbytes, hipMemcpyDeviceToHost));
    if (rc == FDTD_OK) SX(hipMemcpy(st_h.data(), d_st, (size_t)ncell, hipMemcpyDeviceToHost));
  }
  if (rc == FDTD_OK && method == FDTD_SAR_IEEE) {
    double hmax = -1.0;
    bool used = false;
    for (size_t q = 0; q < (size_t)ncell; ++q) {
      if (st_h[q] == FDTD_SAR_VALID && half_h[q] > hmax) hmax = half_h[q];
      used = used || st_h[q] == FDTD_SAR_USED;
    }
    if (used) {                                                     // hmax < 0: no valid cube, every used voxel ends without one
      SecondArgs s{ncx, ncy, ncz, d_lines + co[0], d_lines + co[1], d_lines + co[2], hmax, d_cell + 3 * ncell, d_cell + 2 * ncell, d_st};
      hipLaunchKernelGGL(k_sar_second, dim3((unsigned)((ncell + SAR_BLOCK - 1) / SAR_BLOCK)), dim3(SAR_BLOCK), 0, 0, s);
      SX(hipGetLastError());
      SX(hipDeviceSynchronize());
      if (rc == FDTD_OK) SX(hipMemcpy(st_h.data(), d_st, (size_t)ncell, hipMemcpyDeviceToHost));
    }
  }
  if (rc == FDTD_OK) SX(hipMemcpy(sar_avg, d_cell + 2 * ncell, cbytes, hipMemcpyDeviceToHost));
  if (rc == FDTD_OK) {
    for (int q = 0; q < 4; ++q) counts[q] = 0;
    for (size_t q = 0; q < (size_t)ncell; ++q) {
      half_side[q] = half_h[q];
      status[q] = st_h[q];
      if (st_h[q] >= 0 && st_h[q] < 4) counts[st_h[q]]++;
    }
  }
  hipFree(d_lines); hipFree(d_cell); hipFree(d_st);
  return rc;
}
#undef SX
