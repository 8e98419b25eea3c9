// fields.hip — field dumps: E, H, J and rot-H of a box on a point lattice (include/fdtd_hip_fields.h; fields.py is the specification
// and spells the rules).  Stateless: host pointers in, host pointers out, no context, none of the step schedules.
//
// k_field_interp<KIND, MODE>: one thread per output point, x fastest; the thread writes the three components (and both parts of a
// spectrum), each a run of 8- or 16-byte values along x, so the stores coalesce.  float64 in the association fields.py spells
// (-ffp-contract=off keeps the compiler from fusing), so the output has the specification's bits.  Every read of a recorded array
// goes through ld(), which answers 0 outside the recorded region; an edge or face that does not exist is 0 before any read.  Kind,
// mode and component are template parameters: the axis a rule shifts along is known at compile time and no index lives in memory.
#include <math.h>
#include <stdint.h>

#include <vector>

#include "fdtd_ctx.h"
#include "../../include/fdtd_hip_fields.h"

namespace {
constexpr int FIELD_BLOCK = 256;

struct FieldArgs {
  int P;                  // 1: real samples, 2: (re, im)
  int n[3];               // grid nodes
  int lo[3], sub[3], on[3];
  int rlo[3], rn[3];      // the recorded region: first node and extent
  const double* d[3];     // primal edge lengths, n[a] each (the last repeats)
  const double* dd[3];    // dual edge lengths
  const double* src[3];   // [rn2][rn1][rn0][P]
  const double* kap[3];   // [rn2][rn1][rn0]
  double* out;            // [3][on2][on1][on0][P]
};

template <int A> __device__ __forceinline__ int pick(int x, int y, int z) { return A == 0 ? x : A == 1 ? y : z; }

__device__ __forceinline__ bool in_grid(const FieldArgs& a, int x, int y, int z) {
  return x >= 0 && y >= 0 && z >= 0 && x < a.n[0] && y < a.n[1] && z < a.n[2];
}
template <int C> __device__ __forceinline__ bool edge_exists(const FieldArgs& a, int x, int y, int z) {
  return in_grid(a, x, y, z) && pick<C>(x, y, z) < a.n[C] - 1;
}
template <int C> __device__ __forceinline__ bool face_exists(const FieldArgs& a, int x, int y, int z) {
  constexpr int A1 = (C + 1) % 3, A2 = (C + 2) % 3;
  return in_grid(a, x, y, z) && pick<A1>(x, y, z) < a.n[A1] - 1 && pick<A2>(x, y, z) < a.n[A2] - 1;
}

// A[node (x, y, z)][p] of an array over the recorded region; 0 outside it
__device__ __forceinline__ double ld(const FieldArgs& a, const double* __restrict__ A, int x, int y, int z, int p, int P) {
  const int rx = x - a.rlo[0], ry = y - a.rlo[1], rz = z - a.rlo[2];
  if (rx < 0 || ry < 0 || rz < 0 || rx >= a.rn[0] || ry >= a.rn[1] || rz >= a.rn[2]) return 0.0;
  return A[(((size_t)rz * (size_t)a.rn[1] + (size_t)ry) * (size_t)a.rn[0] + (size_t)rx) * (size_t)P + (size_t)p];
}

template <int C> __device__ __forceinline__ double face_current(const FieldArgs& a, int x, int y, int z, int p) {
  return face_exists<C>(a, x, y, z) ? ld(a, a.src[C], x, y, z, p, a.P) : 0.0;
}

// the raw field of component C at node (x, y, z): fields.py, "Raw fields"
template <int KIND, int C> __device__ __forceinline__ double raw_field(const FieldArgs& a, int x, int y, int z, int p) {
  constexpr int A1 = (C + 1) % 3, A2 = (C + 2) % 3;
  if (KIND == FDTD_FIELD_H) {
    if (!face_exists<C>(a, x, y, z)) return 0.0;
    return ld(a, a.src[C], x, y, z, p, a.P) / a.dd[C][pick<C>(x, y, z)];
  }
  if (!edge_exists<C>(a, x, y, z)) return 0.0;
  if (KIND == FDTD_FIELD_E) return ld(a, a.src[C], x, y, z, p, a.P) / a.d[C][pick<C>(x, y, z)];
  if (KIND == FDTD_FIELD_J) {
    const double e = ld(a, a.src[C], x, y, z, p, a.P) / a.d[C][pick<C>(x, y, z)];
    return ld(a, a.kap[C], x, y, z, 0, 1) * e;
  }
  const double i0 = face_current<A2>(a, x, y, z, p);
  const double i1 = face_current<A2>(a, x - (A1 == 0), y - (A1 == 1), z - (A1 == 2), p);
  const double i2 = face_current<A1>(a, x, y, z, p);
  const double i3 = face_current<A1>(a, x - (A2 == 0), y - (A2 == 1), z - (A2 == 2), p);
  const double cur = ((i0 - i1) - i2) + i3;
  return cur / (a.dd[A1][pick<A1>(x, y, z)] * a.dd[A2][pick<A2>(x, y, z)]);
}

__device__ __forceinline__ double edge_len(const FieldArgs& a, const double* __restrict__ d, int n, int i) {
  return d[min(max(i, 0), n - 1)];
}

template <int KIND, int MODE, int C> __device__ __forceinline__ double point_field(const FieldArgs& a, int x, int y, int z, int p) {
  constexpr int A1 = (C + 1) % 3, A2 = (C + 2) % 3;
  constexpr int c0 = C == 0, c1 = C == 1, c2 = C == 2;
  constexpr int u0 = A1 == 0, u1 = A1 == 1, u2 = A1 == 2;          // e_a1
  constexpr int v0 = A2 == 0, v1 = A2 == 1, v2 = A2 == 2;          // e_a2
  if (MODE == FDTD_FIELD_RAW) return raw_field<KIND, C>(a, x, y, z, p);
  if (MODE == FDTD_FIELD_NODE) {
    if (KIND == FDTD_FIELD_H) {
      const double f00 = raw_field<KIND, C>(a, x, y, z, p), f10 = raw_field<KIND, C>(a, x - u0, y - u1, z - u2, p);
      const double f01 = raw_field<KIND, C>(a, x - v0, y - v1, z - v2, p);
      const double f11 = raw_field<KIND, C>(a, x - u0 - v0, y - u1 - v1, z - u2 - v2, p);
      return 0.25 * ((f00 + f10) + (f01 + f11));
    }
    const int g = pick<C>(x, y, z);
    const double dm = edge_len(a, a.d[C], a.n[C], g - 1), dp = edge_len(a, a.d[C], a.n[C], g);
    const double fm = raw_field<KIND, C>(a, x - c0, y - c1, z - c2, p), fp = raw_field<KIND, C>(a, x, y, z, p);
    return (fm * dp + fp * dm) / (dm + dp);
  }
  if (KIND == FDTD_FIELD_H) return 0.5 * (raw_field<KIND, C>(a, x, y, z, p) + raw_field<KIND, C>(a, x + c0, y + c1, z + c2, p));
  const double a0 = raw_field<KIND, C>(a, x, y, z, p), a1 = raw_field<KIND, C>(a, x + u0, y + u1, z + u2, p);
  const double a2 = raw_field<KIND, C>(a, x + v0, y + v1, z + v2, p);
  const double a3 = raw_field<KIND, C>(a, x + u0 + v0, y + u1 + v1, z + u2 + v2, p);
  return 0.25 * ((a0 + a1) + (a2 + a3));
}

template <int KIND, int MODE> __global__ __launch_bounds__(FIELD_BLOCK) void k_field_interp(const FieldArgs a) {
  const long long q = (long long)blockIdx.x * FIELD_BLOCK + threadIdx.x;
  const long long npts = (long long)a.on[0] * a.on[1] * a.on[2];
  if (q >= npts) return;
  const int ox = (int)(q % a.on[0]), oy = (int)((q / a.on[0]) % a.on[1]), oz = (int)(q / ((long long)a.on[0] * a.on[1]));
  const int x = a.lo[0] + ox * a.sub[0], y = a.lo[1] + oy * a.sub[1], z = a.lo[2] + oz * a.sub[2];
  const size_t P = (size_t)a.P;
  for (int p = 0; p < a.P; ++p) {
    a.out[((size_t)q) * P + p] = point_field<KIND, MODE, 0>(a, x, y, z, p);
    a.out[((size_t)npts + (size_t)q) * P + p] = point_field<KIND, MODE, 1>(a, x, y, z, p);
    a.out[(2 * (size_t)npts + (size_t)q) * P + p] = point_field<KIND, MODE, 2>(a, x, y, z, p);
  }
}

template <int KIND> void launch_mode(int mode, unsigned blocks, const FieldArgs& a) {
  if (mode == FDTD_FIELD_RAW) hipLaunchKernelGGL((k_field_interp<KIND, FDTD_FIELD_RAW>), dim3(blocks), dim3(FIELD_BLOCK), 0, 0, a);
  else if (mode == FDTD_FIELD_NODE) hipLaunchKernelGGL((k_field_interp<KIND, FDTD_FIELD_NODE>), dim3(blocks), dim3(FIELD_BLOCK), 0, 0, a);
  else hipLaunchKernelGGL((k_field_interp<KIND, FDTD_FIELD_CELL>), dim3(blocks), dim3(FIELD_BLOCK), 0, 0, a);
}

bool lines_ok(int n, const double* l) {
  for (int q = 0; q < n; ++q)
    if (!isfinite(l[q]) || (q && !(l[q] > l[q - 1]))) return false;
  return true;
}
}  // namespace

#define FX(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess && rc == FDTD_OK) rc = fdtd_fail(nullptr, e_ == hipErrorOutOfMemory ? FDTD_E_NOMEM : FDTD_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); } while (0)

extern "C" int fdtd_field_interp(int device, int kind, int mode, int parts, const int* n, const int* lo, const int* hi, const int* sub,
                                 const double* x, const double* y, const double* z, const double* rec0, const double* rec1,
                                 const double* rec2, const double* kap0, const double* kap1, const double* kap2, double* out) {
  if (kind < FDTD_FIELD_E || kind > FDTD_FIELD_ROTH || mode < FDTD_FIELD_RAW || mode > FDTD_FIELD_CELL || (parts != 1 && parts != 2) ||
      !n || !lo || !hi || !sub || !x || !y || !z || !rec0 || !rec1 || !rec2 || !out ||
      (kind == FDTD_FIELD_J && (!kap0 || !kap1 || !kap2)))
    return fdtd_fail(nullptr, FDTD_E_ARG, "bad field_interp argument");
  const double* lines[3] = {x, y, z};
  FieldArgs a{};
  a.P = parts;
  long long npts = 1, nreg = 1;
  size_t ntab = 0;
  for (int q = 0; q < 3; ++q) {
    if (n[q] < 2 || !lines_ok(n[q], lines[q]))
      return fdtd_fail(nullptr, FDTD_E_ARG, "field_interp: the node lines must be finite, >= 2 per axis and strictly increasing");
    if (lo[q] < 0 || hi[q] < lo[q] || hi[q] > n[q] - 1 || sub[q] < 1)
      return fdtd_fail(nullptr, FDTD_E_ARG, "field_interp: the box %d..%d (stride %d) along axis %d does not lie in the grid (0..%d)", lo[q],
                       hi[q], sub[q], q, n[q] - 1);
    const int ext = hi[q] - lo[q] + (mode == FDTD_FIELD_CELL ? 0 : 1);
    if (ext < 1) return fdtd_fail(nullptr, FDTD_E_ARG, "field_interp: cell interpolation needs at least one cell along axis %d", q);
    a.n[q] = n[q]; a.lo[q] = lo[q]; a.sub[q] = sub[q];
    a.on[q] = (ext - 1) / sub[q] + 1;
    a.rlo[q] = lo[q] > 0 ? lo[q] - 1 : 0;
    a.rn[q] = hi[q] - a.rlo[q] + 1;
    npts *= a.on[q];
    nreg *= a.rn[q];
    ntab += (size_t)n[q];
  }
  if (nreg * parts >= (1LL << 31)) return fdtd_fail(nullptr, FDTD_E_ARG, "field_interp: the region has %lld values per component, at most 2^31 - 1", nreg * parts);
  // primal and dual edge lengths as grid.RectGrid holds them: [d_x d_y d_z | dd_x dd_y dd_z]
  std::vector<double> tab;
  try {
    tab.resize(2 * ntab);
  } catch (...) {
    return fdtd_fail(nullptr, FDTD_E_NOMEM, "field_interp: no host memory for the metric tables");
  }
  size_t off[3];
  for (size_t q = 0, o = 0; q < 3; o += (size_t)n[q], ++q) {
    off[q] = o;
    const double* l = lines[q];
    const int m = n[q];
    double *d = tab.data() + o, *dd = tab.data() + ntab + o;
    for (int i = 0; i < m - 1; ++i) d[i] = l[i + 1] - l[i];
    d[m - 1] = d[m - 2];
    for (int i = 1; i < m - 1; ++i) dd[i] = 0.5 * (l[i + 1] - l[i - 1]);
    dd[0] = l[1] - l[0];
    dd[m - 1] = l[m - 1] - l[m - 2];
  }
  int rc = FDTD_OK;
  HIPCK(nullptr, hipSetDevice(device));
  const double* rec[3] = {rec0, rec1, rec2};
  const double* kap[3] = {kap0, kap1, kap2};
  double *d_tab = nullptr, *d_src = nullptr, *d_kap = nullptr, *d_out = nullptr;
  const size_t sbytes = (size_t)nreg * (size_t)parts * sizeof(double), kbytes = (size_t)nreg * sizeof(double);
  const size_t obytes = 3 * (size_t)npts * (size_t)parts * sizeof(double);
  FX(hipMalloc(&d_tab, tab.size() * sizeof(double)));
  FX(hipMalloc(&d_src, 3 * sbytes));
  if (kind == FDTD_FIELD_J) FX(hipMalloc(&d_kap, 3 * kbytes));
  FX(hipMalloc(&d_out, obytes));
  if (rc == FDTD_OK) {
    FX(hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    for (int c = 0; c < 3; ++c) FX(hipMemcpy(d_src + (size_t)c * nreg * parts, rec[c], sbytes, hipMemcpyHostToDevice));
    if (kind == FDTD_FIELD_J)
      for (int c = 0; c < 3; ++c) FX(hipMemcpy(d_kap + (size_t)c * nreg, kap[c], kbytes, hipMemcpyHostToDevice));
  }
  if (rc == FDTD_OK) {
    for (int c = 0; c < 3; ++c) {
      a.d[c] = d_tab + off[c];
      a.dd[c] = d_tab + ntab + off[c];
      a.src[c] = d_src + (size_t)c * nreg * parts;
      a.kap[c] = d_kap ? d_kap + (size_t)c * nreg : nullptr;
    }
    a.out = d_out;
    const unsigned blocks = (unsigned)((npts + FIELD_BLOCK - 1) / FIELD_BLOCK);
    if (kind == FDTD_FIELD_E) launch_mode<FDTD_FIELD_E>(mode, blocks, a);
    else if (kind == FDTD_FIELD_H) launch_mode<FDTD_FIELD_H>(mode, blocks, a);
    else if (kind == FDTD_FIELD_J) launch_mode<FDTD_FIELD_J>(mode, blocks, a);
    else launch_mode<FDTD_FIELD_ROTH>(mode, blocks, a);
    FX(hipGetLastError());
    FX(hipDeviceSynchronize());
    if (rc == FDTD_OK) FX(hipMemcpy(out, d_out, obytes, hipMemcpyDeviceToHost));
  }
  hipFree(d_tab); hipFree(d_src); hipFree(d_kap); hipFree(d_out);
  return rc;
}
#undef FX
