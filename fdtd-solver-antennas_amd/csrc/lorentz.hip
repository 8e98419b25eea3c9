// lorentz.hip — Lorentz and Drude media: resonant dielectrics as series R-L-C branches across the edge capacitance
// (include/fdtd_hip_lorentz.h).
//
// The part of the branch currents that is proportional to the mean edge voltage (g0) is folded into the cells' kappa when the
// operator is built; what is left is a correction of every dispersive edge once per timestep, behind the Debye media's and in front
// of the sheets'.  The branch is the series element of lumped.hip, the set of edges the volume of dispersion.hip: per field component
// one dense box of edges laid out like the field arrays, one thread per four consecutive x-edges of a row, every array moved as
// 16-byte vectors, consecutive lanes on consecutive memory, no index array.  Per edge the kernel moves 8 (V) + 4 (vi) + 4 (w) +
// 8 (v_prev) + 16 K (j_k, u_k) bytes and does 17 K + 5 flops: it is a streaming kernel.  Every statement is one fp32 operation in the
// order the header spells (-ffp-contract=off), so a host restatement on top of the oracle's half-steps reproduces it bit for bit.
#include "fdtd_ctx.h"
#include "kernel_common.hpp"
#include "../../include/fdtd_hip_lorentz.h"

#include <vector>

namespace {

constexpr int ROW = 8;                                                  // floats per (medium, pole): phi00 phi01 phi10 phi11 gam0 gam1 h0 h1
constexpr int MROW = FDTD_LORENTZ_MAX_K * ROW;                          // floats per medium
constexpr int TAB = FDTD_LORENTZ_MAX_MEDIA * MROW;                      // floats of the whole table
static_assert(TAB == 256, "k_lorentz loads the table with one float per thread of a 256-thread block");

struct LorentzComp {
  float* V;                // the component's voltage array (local plane 0)
  const float* w; const float* vi; const uint8_t* med;
  float* vprev; float* x;
  unsigned blk0;           // first block of this component in the launch
  unsigned nq;             // threads = groups of four x-edges: nz_b * ny_b * qx
  unsigned n;              // edges of the widened box = 4 * nq (stride of the state planes)
  int off0;                // field offset of the box's first edge: z0 * plane + y0 * P + x0w
  FastDiv fd_qx, fd_ny;    // groups per row, rows per plane
};
struct LorentzArgs { LorentzComp c[3]; int K, P, plane; const float* tab; };

// One lane of the correction (the header's statement list); t: the rows of the edge's medium.  w == 0: nothing changes.
template <int KMAX>
__device__ __forceinline__ void lorentz_edge(float& V, float& vp, float (&xj)[KMAX], float (&xu)[KMAX], const int K, const float w,
                                             const float vi, const float* t) {
  float S = 0.0f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < K) {
      const float p0 = t[k * ROW + 6] * xj[k];
      const float p1 = t[k * ROW + 7] * xu[k];
      const float s = p0 + p1;
      S = S + s;
    }
  }
  const float tt = w * S;
  const float q = vi * tt;
  const float vn = V - q;
  const float s = vn + vp;
  const float avg = 0.5f * s;
  const bool on = w != 0.0f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < K) {
      const float* r = t + k * ROW;
      const float a0 = r[0] * xj[k];
      const float b0 = r[1] * xu[k];
      const float c0 = a0 + b0;
      const float d0 = r[4] * avg;
      const float jn = c0 + d0;
      const float a1 = r[2] * xj[k];
      const float b1 = r[3] * xu[k];
      const float c1 = a1 + b1;
      const float d1 = r[5] * avg;
      const float un = c1 + d1;
      xj[k] = on ? jn : xj[k];
      xu[k] = on ? un : xu[k];
    }
  }
  V = on ? vn : V;
  vp = on ? vn : vp;
}

// MULTI: several media — the table sits in LDS and every lane looks its edge's medium up; else the one medium's rows are
// wave-uniform (scalar loads).  KMAX: compile-time bound of the pole loops (1: a plasma or one resonance, 2, 4: everything).
template <bool MULTI, int KMAX>
__global__ __launch_bounds__(256) void k_lorentz(const LorentzArgs a) {
  __shared__ float tab[MULTI ? TAB : 1];
  if (MULTI) {
    tab[threadIdx.x] = a.tab[threadIdx.x];
    __syncthreads();
  }
  const unsigned b = blockIdx.x;
  const int ci = b >= a.c[2].blk0 ? 2 : b >= a.c[1].blk0 ? 1 : 0;
  const LorentzComp& d = a.c[ci];
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
  float jx[KMAX], jy_[KMAX], jz[KMAX], jw[KMAX], ux[KMAX], uy[KMAX], uz[KMAX], uw[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k < K) {
      const float4 tj = *reinterpret_cast<const float4*>(d.x + (size_t)(2 * k) * d.n + o);
      const float4 tu = *reinterpret_cast<const float4*>(d.x + (size_t)(2 * k + 1) * d.n + o);
      jx[k] = tj.x; jy_[k] = tj.y; jz[k] = tj.z; jw[k] = tj.w;
      ux[k] = tu.x; uy[k] = tu.y; uz[k] = tu.z; uw[k] = tu.w;
    } else {
      jx[k] = jy_[k] = jz[k] = jw[k] = ux[k] = uy[k] = uz[k] = uw[k] = 0.0f;
    }
  }
  if (MULTI) {
    const unsigned m4 = *reinterpret_cast<const unsigned*>(d.med + o);
    lorentz_edge<KMAX>(V4.x, vp4.x, jx, ux, K, w4.x, vi4.x, tab + (m4 & 0xffu) * MROW);
    lorentz_edge<KMAX>(V4.y, vp4.y, jy_, uy, K, w4.y, vi4.y, tab + ((m4 >> 8) & 0xffu) * MROW);
    lorentz_edge<KMAX>(V4.z, vp4.z, jz, uz, K, w4.z, vi4.z, tab + ((m4 >> 16) & 0xffu) * MROW);
    lorentz_edge<KMAX>(V4.w, vp4.w, jw, uw, K, w4.w, vi4.w, tab + (m4 >> 24) * MROW);
  } else {
    const float* t = a.tab;
    lorentz_edge<KMAX>(V4.x, vp4.x, jx, ux, K, w4.x, vi4.x, t);
    lorentz_edge<KMAX>(V4.y, vp4.y, jy_, uy, K, w4.y, vi4.y, t);
    lorentz_edge<KMAX>(V4.z, vp4.z, jz, uz, K, w4.z, vi4.z, t);
    lorentz_edge<KMAX>(V4.w, vp4.w, jw, uw, K, w4.w, vi4.w, t);
  }
  *reinterpret_cast<float4*>(d.V + of) = V4;
  *reinterpret_cast<float4*>(d.vprev + o) = vp4;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      *reinterpret_cast<float4*>(d.x + (size_t)(2 * k) * d.n + o) = make_float4(jx[k], jy_[k], jz[k], jw[k]);
      *reinterpret_cast<float4*>(d.x + (size_t)(2 * k + 1) * d.n + o) = make_float4(ux[k], uy[k], uz[k], uw[k]);
    }
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

void lorentz_free(fdtd_ctx* c) {
  for (auto& b : c->lorentz_box) {
    hipFree(b.w); hipFree(b.vi); hipFree(b.vprev); hipFree(b.u); hipFree(b.med);
    b = fdtd_ctx::DebyeBox{};
  }
  hipFree(c->lorentz_tab);
  c->lorentz_tab = nullptr;
  c->lorentz_nmedia = c->lorentz_K = 0;
}

void launch_lorentz(fdtd_ctx* c, hipStream_t s) {
  if (c->lorentz_nmedia <= 0) return;
  LorentzArgs a{};
  unsigned blocks = 0;
  for (int ci = 0; ci < 3; ++ci) {
    const fdtd_ctx::DebyeBox& b = c->lorentz_box[ci];
    LorentzComp& d = a.c[ci];
    d.blk0 = blocks;
    d.nq = (unsigned)(b.n / 4);
    d.n = (unsigned)b.n;
    d.fd_qx = make_fastdiv(1); d.fd_ny = make_fastdiv(1);
    if (b.n == 0) continue;
    d.V = c->p.V[ci]; d.w = b.w; d.vi = b.vi; d.med = b.med; d.vprev = b.vprev; d.x = b.u;
    d.off0 = b.lo[2] * c->plane + b.lo[1] * c->P + b.x0w;
    d.fd_qx = make_fastdiv((unsigned)(b.nxw / 4));
    d.fd_ny = make_fastdiv((unsigned)(b.hi[1] - b.lo[1]));
    blocks += (d.nq + 255u) / 256u;
  }
  if (blocks == 0) return;
  a.K = c->lorentz_K; a.P = c->P; a.plane = c->plane; a.tab = c->lorentz_tab;
  const bool multi = c->lorentz_nmedia > 1;
  const int kb = c->lorentz_K <= 1 ? 1 : c->lorentz_K <= 2 ? 2 : 4;
  auto kern = multi ? (kb == 1 ? k_lorentz<true, 1> : kb == 2 ? k_lorentz<true, 2> : k_lorentz<true, 4>)
                    : (kb == 1 ? k_lorentz<false, 1> : kb == 2 ? k_lorentz<false, 2> : k_lorentz<false, 4>);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, s, a);
}

extern "C" {

int fdtd_lorentz_set(fdtd_ctx* c, int nmedia, int K, const float* phi, const float* gam, const float* h,
                     const int32_t lo[3][3], const int32_t hi[3][3], const float* const w[3], const uint8_t* const med[3]) {
  if (!c) return FDTD_E_ARG;
  if (nmedia < 0 || nmedia > FDTD_LORENTZ_MAX_MEDIA)
    return fdtd_fail(c, FDTD_E_ARG, "fdtd_lorentz_set: at most %d media", FDTD_LORENTZ_MAX_MEDIA);
  if (nmedia > 0 && (K < 1 || K > FDTD_LORENTZ_MAX_K)) return fdtd_fail(c, FDTD_E_ARG, "fdtd_lorentz_set: K must be 1..%d", FDTD_LORENTZ_MAX_K);
  if (nmedia > 0 && (!phi || !gam || !h || !lo || !hi || !w)) return fdtd_fail(c, FDTD_E_ARG, "fdtd_lorentz_set: bad argument");
  if (nmedia > 0 && (c->d.world > 1 || c->p.p2p || c->link_lo || c->link_hi))
    return fdtd_fail(c, FDTD_E_UNSUPPORTED, "Lorentz media: single slab only (world = 1, no p2p transport, no linked contexts)");
  if (!c->have_op) return fdtd_fail(c, FDTD_E_STATE, "fdtd_lorentz_set: set the operator first");
  if (c->step != 0) return fdtd_fail(c, FDTD_E_STATE, "fdtd_lorentz_set: before the first timestep");
  const int nn[3] = {c->d.nx, c->d.ny, c->d.nz};
  size_t nbox[3] = {0, 0, 0};
  for (int ci = 0; ci < 3 && nmedia > 0; ++ci) {
    bool empty = false;
    for (int a = 0; a < 3; ++a) empty = empty || hi[ci][a] <= lo[ci][a];
    if (empty) continue;
    for (int a = 0; a < 3; ++a)
      if (lo[ci][a] < 0 || hi[ci][a] > (a == ci ? nn[a] - 1 : nn[a]))
        return fdtd_fail(c, FDTD_E_ARG, "fdtd_lorentz_set: component %d: box [%d, %d) along axis %d leaves the grid's edges", ci, lo[ci][a], hi[ci][a], a);
    if (!w[ci] || (nmedia > 1 && (!med || !med[ci]))) return fdtd_fail(c, FDTD_E_ARG, "fdtd_lorentz_set: component %d: weights / medium ids missing", ci);
    nbox[ci] = (size_t)(hi[ci][0] - lo[ci][0]) * (hi[ci][1] - lo[ci][1]) * (hi[ci][2] - lo[ci][2]);
    if (nbox[ci] * 4 > 0x7fffffffu) return fdtd_fail(c, FDTD_E_ARG, "fdtd_lorentz_set: component %d: box too large", ci);
    if (nmedia > 1)
      for (size_t e = 0; e < nbox[ci]; ++e)
        if (med[ci][e] >= nmedia) return fdtd_fail(c, FDTD_E_ARG, "fdtd_lorentz_set: component %d: medium id %d out of range", ci, (int)med[ci][e]);
  }
  HIPCK(c, hipSetDevice(c->d.device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  lorentz_free(c);
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
    fdtd_ctx::DebyeBox& b = c->lorentz_box[ci];
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
          // an edge the operator holds at zero (vi == 0: a grid face, metal) is no dispersive edge (the header; fdtd_debye_set's rule)
          vv[dst + x] = op[1][g + x];
          ww[dst + x] = vv[dst + x] == 0.0f ? 0.0f : w[ci][src + x];
          if (nmedia > 1) mm[dst + x] = med[ci][src + x];
        }
      }
    e = upload(&b.w, ww);
    if (e == hipSuccess) e = upload(&b.vi, vv);
    if (e == hipSuccess && nmedia > 1) e = upload(&b.med, mm);
    if (e == hipSuccess) e = upload(&b.vprev, std::vector<float>(b.n, 0.f));
    if (e == hipSuccess) e = upload(&b.u, std::vector<float>((size_t)2 * K * b.n, 0.f));
  }
  if (e == hipSuccess) {
    std::vector<float> tab(TAB, 0.f);
    for (int m = 0; m < nmedia; ++m)
      for (int k = 0; k < K; ++k) {
        float* row = &tab[(size_t)m * MROW + k * ROW];
        for (int q = 0; q < 4; ++q) row[q] = phi[((size_t)m * K + k) * 4 + q];
        for (int q = 0; q < 2; ++q) { row[4 + q] = gam[((size_t)m * K + k) * 2 + q]; row[6 + q] = h[((size_t)m * K + k) * 2 + q]; }
      }
    e = upload(&c->lorentz_tab, tab);
  }
  if (e != hipSuccess) {
    lorentz_free(c);
    return fdtd_fail(c, e == hipErrorOutOfMemory ? FDTD_E_NOMEM : FDTD_E_DEVICE, "fdtd_lorentz_set: %s", hipGetErrorString(e));
  }
  c->lorentz_nmedia = nmedia; c->lorentz_K = K;
  return FDTD_OK;
}

int fdtd_lorentz_get(fdtd_ctx* c, int comp, float* v_prev, float* x, float* vi) {
  if (!c) return FDTD_E_ARG;
  if (comp < 0 || comp > 2) return fdtd_fail(c, FDTD_E_ARG, "fdtd_lorentz_get: component %d", comp);
  HIPCK(c, hipSetDevice(c->d.device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  const fdtd_ctx::DebyeBox& b = c->lorentz_box[comp];
  if (c->lorentz_nmedia == 0 || b.n == 0) return FDTD_OK;
  const int nyb = b.hi[1] - b.lo[1], nzb = b.hi[2] - b.lo[2], nxb = b.hi[0] - b.lo[0];
  const size_t rows = (size_t)nyb * nzb;
  const size_t x0 = (size_t)(b.lo[0] - b.x0w);
  std::vector<float> tmp(b.n);
  auto crop = [&](const float* dev, float* out) -> hipError_t {
    hipError_t e = hipMemcpy(tmp.data(), dev, b.n * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (size_t r = 0; r < rows; ++r)
      for (int xx = 0; xx < nxb; ++xx) out[r * nxb + xx] = tmp[r * b.nxw + x0 + xx];
    return hipSuccess;
  };
  if (v_prev) HIPCK(c, crop(b.vprev, v_prev));
  if (vi) HIPCK(c, crop(b.vi, vi));
  if (x)
    for (int p = 0; p < 2 * c->lorentz_K; ++p) HIPCK(c, crop(b.u + (size_t)p * b.n, x + (size_t)p * rows * nxb));
  return FDTD_OK;
}

}  // extern "C"
