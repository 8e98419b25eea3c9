// dispersion.hip — Debye media: dispersive dielectrics as R-C branches across the edge capacitance (include/fdtd_hip_dispersion.h).
//
// The part of the branch currents that is proportional to the mean edge voltage is folded into the cells' kappa when the operator
// is built; what is left is a correction of every dispersive edge once per timestep, between the E phase and the H update.  Unlike
// the conducting sheets' correction it is a VOLUME effect (a substrate a few cells thick is ~1e6 edges with K states each), so it
// is dense: per field component one box of edges laid out like the field arrays, one thread per four consecutive x-edges of a row,
// every array moved as 16-byte vectors, consecutive lanes on consecutive memory, no index array.  Per edge the kernel moves
// 8 (V) + 4 (vi) + 4 (w) + 8 (v_prev) + 8 K (u) bytes and does 5 K + 4 flops: it is a streaming kernel.  Every statement is one
// fp32 operation in the order the header spells (-ffp-contract=off), so a host restatement on top of the oracle's half-steps
// reproduces it bit for bit.
#include "fdtd_ctx.h"
#include "kernel_common.hpp"
#include "../../include/fdtd_hip_dispersion.h"

#include <vector>

namespace {

constexpr int TAB = FDTD_DEBYE_MAX_MEDIA * FDTD_DEBYE_MAX_K;   // floats per table (alpha / oma / beta), [medium][MAX_K]

struct DebyeComp {
  float* V;                // the component's voltage array (local plane 0)
  const float* w; const float* vi; const uint8_t* med;
  float* vprev; float* u;
  unsigned blk0;           // first block of this component in the launch
  unsigned nq;             // threads = groups of four x-edges: nz_b * ny_b * qx
  unsigned n;              // edges of the widened box = 4 * nq (stride of the u planes)
  int off0;                // field offset of the box's first edge: z0 * plane + y0 * P + x0w
  FastDiv fd_qx, fd_ny;    // groups per row, rows per plane
};
struct DebyeArgs { DebyeComp c[3]; int K, P, plane; const float* tab; };

// One lane of the correction (the header's statement list).  w == 0: nothing changes.
template <int KMAX>
__device__ __forceinline__ void debye_edge(float& V, float& vp, float (&u)[KMAX], const int K, const float w, const float vi,
                                           const float* al, const float* om, const float* be) {
  float S = 0.0f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < K) {
      const float t = w * be[k];
      const float p = t * u[k];
      S = S + p;
    }
  }
  const float q = vi * S;
  const float vn = V + q;
  const float s = vn + vp;
  const float avg = 0.5f * s;
  const bool on = w != 0.0f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < K) {
      const float a = al[k] * u[k];
      const float b = om[k] * avg;
      const float un = a + b;
      u[k] = on ? un : u[k];
    }
  }
  V = on ? vn : V;
  vp = on ? vn : vp;
}

// MULTI: several media — the tables sit in LDS and every lane looks its edge's medium up; else the one medium's rows are
// wave-uniform (scalar loads).  KMAX: compile-time bound of the pole loops (4 covers the fitted substrates, 8 everything).
template <bool MULTI, int KMAX>
__global__ __launch_bounds__(256) void k_debye(const DebyeArgs a) {
  __shared__ float tab[MULTI ? 3 * TAB : 1];
  if (MULTI) {
    if (threadIdx.x < 3 * TAB) tab[threadIdx.x] = a.tab[threadIdx.x];
    __syncthreads();
  }
  const unsigned b = blockIdx.x;
  const int ci = b >= a.c[2].blk0 ? 2 : b >= a.c[1].blk0 ? 1 : 0;
  const DebyeComp& d = a.c[ci];
  const unsigned q = (b - d.blk0) * 256u + threadIdx.x;
  if (q >= d.nq) return;
  const unsigned row = fd_div(q, d.fd_qx);
  const unsigned ix = q - row * d.fd_qx.d;
  const unsigned kz = fd_div(row, d.fd_ny);
  const unsigned jy = row - kz * d.fd_ny.d;
  const size_t o = (size_t)q * 4u;                                                     // in the box arrays
  const long of = (long)d.off0 + (long)kz * a.plane + (long)jy * a.P + (long)ix * 4;   // in the field array
  const float4 w4 = *reinterpret_cast<const float4*>(d.w + o);
  if (w4.x == 0.0f && w4.y == 0.0f && w4.z == 0.0f && w4.w == 0.0f) return;   // (padding, or cells of another material inside the box)
  const float4 vi4 = *reinterpret_cast<const float4*>(d.vi + o);
  float4 V4 = *reinterpret_cast<const float4*>(d.V + of);
  float4 vp4 = *reinterpret_cast<const float4*>(d.vprev + o);
  const int K = a.K;
  float ux[KMAX], uy[KMAX], uz[KMAX], uw[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < K) {
      const float4 t = *reinterpret_cast<const float4*>(d.u + (size_t)k * d.n + o);
      ux[k] = t.x; uy[k] = t.y; uz[k] = t.z; uw[k] = t.w;
    } else {
      ux[k] = uy[k] = uz[k] = uw[k] = 0.0f;
    }
  }
  if (MULTI) {
    const unsigned m4 = *reinterpret_cast<const unsigned*>(d.med + o);
    const float* t0 = tab + (m4 & 0xffu) * FDTD_DEBYE_MAX_K;
    const float* t1 = tab + ((m4 >> 8) & 0xffu) * FDTD_DEBYE_MAX_K;
    const float* t2 = tab + ((m4 >> 16) & 0xffu) * FDTD_DEBYE_MAX_K;
    const float* t3 = tab + (m4 >> 24) * FDTD_DEBYE_MAX_K;
    debye_edge<KMAX>(V4.x, vp4.x, ux, K, w4.x, vi4.x, t0, t0 + TAB, t0 + 2 * TAB);
    debye_edge<KMAX>(V4.y, vp4.y, uy, K, w4.y, vi4.y, t1, t1 + TAB, t1 + 2 * TAB);
    debye_edge<KMAX>(V4.z, vp4.z, uz, K, w4.z, vi4.z, t2, t2 + TAB, t2 + 2 * TAB);
    debye_edge<KMAX>(V4.w, vp4.w, uw, K, w4.w, vi4.w, t3, t3 + TAB, t3 + 2 * TAB);
  } else {
    const float* t = a.tab;
    debye_edge<KMAX>(V4.x, vp4.x, ux, K, w4.x, vi4.x, t, t + TAB, t + 2 * TAB);
    debye_edge<KMAX>(V4.y, vp4.y, uy, K, w4.y, vi4.y, t, t + TAB, t + 2 * TAB);
    debye_edge<KMAX>(V4.z, vp4.z, uz, K, w4.z, vi4.z, t, t + TAB, t + 2 * TAB);
    debye_edge<KMAX>(V4.w, vp4.w, uw, K, w4.w, vi4.w, t, t + TAB, t + 2 * TAB);
  }
  *reinterpret_cast<float4*>(d.V + of) = V4;
  *reinterpret_cast<float4*>(d.vprev + o) = vp4;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) *reinterpret_cast<float4*>(d.u + (size_t)k * d.n + o) = make_float4(ux[k], uy[k], uz[k], uw[k]);
}

template <class T>
hipError_t upload(T** dst, const std::vector<T>& v) {
  hipError_t e = hipMalloc((void**)dst, v.size() * sizeof(T));
  if (e == hipSuccess) e = hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  return e;
}

inline int floor4(int v) { return v & ~3; }
inline int ceil4(int v) { return (v + 3) & ~3; }

}  // namespace

void debye_free(fdtd_ctx* c) {
  for (auto& b : c->debye_box) {
    hipFree(b.w); hipFree(b.vi); hipFree(b.vprev); hipFree(b.u); hipFree(b.med);
    b = fdtd_ctx::DebyeBox{};
  }
  hipFree(c->debye_tab);
  c->debye_tab = nullptr;
  c->debye_nmedia = c->debye_K = 0;
}

void launch_debye(fdtd_ctx* c, hipStream_t s) {
  if (c->debye_nmedia <= 0) return;
  DebyeArgs a{};
  unsigned blocks = 0;
  for (int ci = 0; ci < 3; ++ci) {
    const fdtd_ctx::DebyeBox& b = c->debye_box[ci];
    DebyeComp& d = a.c[ci];
    d.blk0 = blocks;
    d.nq = (unsigned)(b.n / 4);
    d.n = (unsigned)b.n;
    d.fd_qx = make_fastdiv(1); d.fd_ny = make_fastdiv(1);
    if (b.n == 0) continue;
    d.V = c->p.V[ci]; d.w = b.w; d.vi = b.vi; d.med = b.med; d.vprev = b.vprev; d.u = b.u;
    d.off0 = b.lo[2] * c->plane + b.lo[1] * c->P + b.x0w;
    d.fd_qx = make_fastdiv((unsigned)(b.nxw / 4));
    d.fd_ny = make_fastdiv((unsigned)(b.hi[1] - b.lo[1]));
    blocks += (d.nq + 255u) / 256u;
  }
  if (blocks == 0) return;
  a.K = c->debye_K; a.P = c->P; a.plane = c->plane; a.tab = c->debye_tab;
  const bool multi = c->debye_nmedia > 1;
  const bool k4 = c->debye_K <= 4;
  auto kern = multi ? (k4 ? k_debye<true, 4> : k_debye<true, 8>) : (k4 ? k_debye<false, 4> : k_debye<false, 8>);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, s, a);
}

extern "C" {

int fdtd_debye_set(fdtd_ctx* c, int nmedia, int K, const float* alpha, const float* oma, const float* beta,
                   const int32_t lo[3][3], const int32_t hi[3][3], const float* const w[3], const uint8_t* const med[3]) {
  if (!c) return FDTD_E_ARG;
  if (nmedia < 0 || nmedia > FDTD_DEBYE_MAX_MEDIA)
    return fdtd_fail(c, FDTD_E_ARG, "fdtd_debye_set: at most %d media", FDTD_DEBYE_MAX_MEDIA);
  if (nmedia > 0 && (K < 1 || K > FDTD_DEBYE_MAX_K)) return fdtd_fail(c, FDTD_E_ARG, "fdtd_debye_set: K must be 1..%d", FDTD_DEBYE_MAX_K);
  if (nmedia > 0 && (!alpha || !oma || !beta || !lo || !hi || !w)) return fdtd_fail(c, FDTD_E_ARG, "fdtd_debye_set: bad argument");
  if (nmedia > 0 && (c->d.world > 1 || c->p.p2p || c->link_lo || c->link_hi))
    return fdtd_fail(c, FDTD_E_UNSUPPORTED, "Debye media: single slab only (world = 1, no p2p transport, no linked contexts)");
  if (!c->have_op) return fdtd_fail(c, FDTD_E_STATE, "fdtd_debye_set: set the operator first");
  if (c->step != 0) return fdtd_fail(c, FDTD_E_STATE, "fdtd_debye_set: before the first timestep");
  const int nn[3] = {c->d.nx, c->d.ny, c->d.nz};
  size_t nbox[3] = {0, 0, 0};
  for (int ci = 0; ci < 3 && nmedia > 0; ++ci) {
    bool empty = false;
    for (int a = 0; a < 3; ++a) empty = empty || hi[ci][a] <= lo[ci][a];
    if (empty) continue;
    for (int a = 0; a < 3; ++a)
      if (lo[ci][a] < 0 || hi[ci][a] > (a == ci ? nn[a] - 1 : nn[a]))
        return fdtd_fail(c, FDTD_E_ARG, "fdtd_debye_set: component %d: box [%d, %d) along axis %d leaves the grid's edges", ci, lo[ci][a], hi[ci][a], a);
    if (!w[ci] || (nmedia > 1 && (!med || !med[ci]))) return fdtd_fail(c, FDTD_E_ARG, "fdtd_debye_set: component %d: weights / medium ids missing", ci);
    nbox[ci] = (size_t)(hi[ci][0] - lo[ci][0]) * (hi[ci][1] - lo[ci][1]) * (hi[ci][2] - lo[ci][2]);
    if (nbox[ci] * 4 > 0x7fffffffu) return fdtd_fail(c, FDTD_E_ARG, "fdtd_debye_set: component %d: box too large", ci);
    if (nmedia > 1)
      for (size_t e = 0; e < nbox[ci]; ++e)
        if (med[ci][e] >= nmedia) return fdtd_fail(c, FDTD_E_ARG, "fdtd_debye_set: component %d: medium id %d out of range", ci, (int)med[ci][e]);
  }
  HIPCK(c, hipSetDevice(c->d.device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  debye_free(c);
  if (nmedia == 0 || nbox[0] + nbox[1] + nbox[2] == 0) return FDTD_OK;
  // the edges' vi, as the update kernels expand it (raw or class form): the whole operator once, cropped to the boxes
  const size_t ncell = (size_t)c->d.nk * c->d.ny * c->d.nx;
  std::vector<float> op[4];
  for (auto& v : op) v.resize(3 * ncell);
  int r = fdtd_get_operator(c, op[0].data(), op[1].data(), op[2].data(), op[3].data());
  if (r) return r;
  hipError_t e = hipSuccess;
  for (int ci = 0; ci < 3 && e == hipSuccess; ++ci) {
    if (nbox[ci] == 0) continue;
    fdtd_ctx::DebyeBox& b = c->debye_box[ci];
    for (int a = 0; a < 3; ++a) { b.lo[a] = lo[ci][a]; b.hi[a] = hi[ci][a]; }
    b.x0w = floor4(b.lo[0]);
    b.nxw = ceil4(b.hi[0]) - b.x0w;           // ceil4(hi) <= ceil4(nx) = P: the widened rows stay inside the field rows
    const int nyb = b.hi[1] - b.lo[1], nzb = b.hi[2] - b.lo[2], nxb = b.hi[0] - b.lo[0];
    b.n = (size_t)b.nxw * nyb * nzb;
    std::vector<float> ww(b.n, 0.f), vv(b.n, 0.f);
    std::vector<uint8_t> mm(b.n, 0);
    for (int z = 0; z < nzb; ++z)
      for (int y = 0; y < nyb; ++y) {
        const size_t src = ((size_t)z * nyb + y) * nxb, dst = ((size_t)z * nyb + y) * b.nxw + (b.lo[0] - b.x0w);
        const size_t g = (size_t)ci * ncell + ((size_t)(b.lo[2] + z) * c->d.ny + (b.lo[1] + y)) * c->d.nx + b.lo[0];
        for (int x = 0; x < nxb; ++x) {
          // an edge the operator holds at zero (vi == 0: a grid face, metal) is no dispersive edge: the correction could never change its
          // voltage, so its states could never act — and on a Mur face the voltage between the two launches is not the timestep's final one
          vv[dst + x] = op[1][g + x];
          ww[dst + x] = vv[dst + x] == 0.0f ? 0.0f : w[ci][src + x];
          if (nmedia > 1) mm[dst + x] = med[ci][src + x];
        }
      }
    e = upload(&b.w, ww);
    if (e == hipSuccess) e = upload(&b.vi, vv);
    if (e == hipSuccess && nmedia > 1) e = upload(&b.med, mm);
    if (e == hipSuccess) e = upload(&b.vprev, std::vector<float>(b.n, 0.f));
    if (e == hipSuccess) e = upload(&b.u, std::vector<float>((size_t)K * b.n, 0.f));
  }
  if (e == hipSuccess) {
    std::vector<float> tab(3 * TAB, 0.f);
    const float* src[3] = {alpha, oma, beta};
    for (int t = 0; t < 3; ++t)
      for (int m = 0; m < nmedia; ++m)
        for (int k = 0; k < K; ++k) tab[(size_t)t * TAB + m * FDTD_DEBYE_MAX_K + k] = src[t][m * K + k];
    e = upload(&c->debye_tab, tab);
  }
  if (e != hipSuccess) {
    debye_free(c);
    return fdtd_fail(c, e == hipErrorOutOfMemory ? FDTD_E_NOMEM : FDTD_E_DEVICE, "fdtd_debye_set: %s", hipGetErrorString(e));
  }
  c->debye_nmedia = nmedia; c->debye_K = K;
  return FDTD_OK;
}

int fdtd_debye_get(fdtd_ctx* c, int comp, float* v_prev, float* u, float* vi) {
  if (!c) return FDTD_E_ARG;
  if (comp < 0 || comp > 2) return fdtd_fail(c, FDTD_E_ARG, "fdtd_debye_get: component %d", comp);
  HIPCK(c, hipSetDevice(c->d.device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  const fdtd_ctx::DebyeBox& b = c->debye_box[comp];
  if (c->debye_nmedia == 0 || b.n == 0) return FDTD_OK;
  const int nyb = b.hi[1] - b.lo[1], nzb = b.hi[2] - b.lo[2], nxb = b.hi[0] - b.lo[0];
  const size_t rows = (size_t)nyb * nzb;
  const size_t x0 = (size_t)(b.lo[0] - b.x0w);
  std::vector<float> tmp(b.n);
  auto crop = [&](const float* dev, float* out) -> hipError_t {
    hipError_t e = hipMemcpy(tmp.data(), dev, b.n * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (size_t r = 0; r < rows; ++r)
      for (int x = 0; x < nxb; ++x) out[r * nxb + x] = tmp[r * b.nxw + x0 + x];
    return hipSuccess;
  };
  if (v_prev) HIPCK(c, crop(b.vprev, v_prev));
  if (vi) HIPCK(c, crop(b.vi, vi));
  if (u)
    for (int k = 0; k < c->debye_K; ++k) HIPCK(c, crop(b.u + (size_t)k * b.n, u + (size_t)k * rows * nxb));
  return FDTD_OK;
}

}  // extern "C"
