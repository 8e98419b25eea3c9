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
#include "dense_box.hpp"
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
  BoxLaunch l;
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
  unsigned q;
  const LorentzComp& d = box_group(a.c, q);
  if (q >= d.l.nq) return;
  const long of = box_field_offset(d.l, q, a.P, a.plane);         // in the field array
  const size_t o = (size_t)q * 4u;                                // in the box arrays
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
      const float4 tj = *reinterpret_cast<const float4*>(d.x + (size_t)(2 * k) * d.l.n + o);
      const float4 tu = *reinterpret_cast<const float4*>(d.x + (size_t)(2 * k + 1) * d.l.n + o);
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
      *reinterpret_cast<float4*>(d.x + (size_t)(2 * k) * d.l.n + o) = make_float4(jx[k], jy_[k], jz[k], jw[k]);
      *reinterpret_cast<float4*>(d.x + (size_t)(2 * k + 1) * d.l.n + o) = make_float4(ux[k], uy[k], uz[k], uw[k]);
    }
}

void launch_lorentz(fdtd_ctx* c, long long, hipStream_t s) {
  const MediaBoxes& m = c->lorentz;
  if (m.nmedia <= 0) return;
  LorentzArgs a{};
  const unsigned blocks = box_layout(c, m.box, a.c);
  if (blocks == 0) return;
  for (int ci = 0; ci < 3; ++ci) {
    const MediaBoxes::Box& b = m.box[ci];
    if (b.g.n == 0) continue;
    LorentzComp& d = a.c[ci];
    d.V = c->p.V[ci]; d.w = b.w; d.vi = b.vi; d.med = b.med; d.vprev = b.vprev; d.x = b.u;
  }
  a.K = m.K; a.P = c->P; a.plane = c->plane; a.tab = m.tab;
  const bool multi = m.nmedia > 1;
  const int kb = m.K <= 1 ? 1 : m.K <= 2 ? 2 : 4;
  auto kern = multi ? (kb == 1 ? k_lorentz<true, 1> : kb == 2 ? k_lorentz<true, 2> : k_lorentz<true, 4>)
                    : (kb == 1 ? k_lorentz<false, 1> : kb == 2 ? k_lorentz<false, 2> : k_lorentz<false, 4>);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, s, a);
}

}  // namespace

#ifndef __HIP_DEVICE_COMPILE__   // (host data: corrections.hpp)
const CorrectionRow corr_lorentz = {
    "Lorentz media", /*no_links*/ true, /*volume*/ true,
    [](const fdtd_ctx* c) { return c->lorentz.nmedia > 0; },
    launch_lorentz, nullptr,
    [](fdtd_ctx* c) { media_free(&c->lorentz); },
    nullptr, nullptr};
#endif

extern "C" {

int fdtd_lorentz_set(fdtd_ctx* c, int nmedia, int K, const float* phi, const float* gam, const float* h,
                     const int32_t lo[3][3], const int32_t hi[3][3], const float* const w[3], const uint8_t* const med[3]) {
  if (!c) return FDTD_E_ARG;
  if (nmedia < 0 || nmedia > FDTD_LORENTZ_MAX_MEDIA)
    return fdtd_fail(c, FDTD_E_ARG, "fdtd_lorentz_set: at most %d media", FDTD_LORENTZ_MAX_MEDIA);
  if (nmedia > 0 && (K < 1 || K > FDTD_LORENTZ_MAX_K)) return fdtd_fail(c, FDTD_E_ARG, "fdtd_lorentz_set: K must be 1..%d", FDTD_LORENTZ_MAX_K);
  if (nmedia > 0 && (!phi || !gam || !h || !lo || !hi || !w)) return fdtd_fail(c, FDTD_E_ARG, "fdtd_lorentz_set: bad argument");
  std::vector<float> tab(TAB, 0.f);
  for (int m = 0; m < nmedia; ++m)
    for (int k = 0; k < K; ++k) {
      float* row = &tab[(size_t)m * MROW + k * ROW];
      for (int q = 0; q < 4; ++q) row[q] = phi[((size_t)m * K + k) * 4 + q];
      for (int q = 0; q < 2; ++q) { row[4 + q] = gam[((size_t)m * K + k) * 2 + q]; row[6 + q] = h[((size_t)m * K + k) * 2 + q]; }
    }
  return media_set(c, &c->lorentz, corr_lorentz, "fdtd_lorentz_set", 2, nmedia, K, tab, lo, hi, w, med);
}

int fdtd_lorentz_get(fdtd_ctx* c, int comp, float* v_prev, float* x, float* vi) {
  if (!c) return FDTD_E_ARG;
  return media_get(c, &c->lorentz, "fdtd_lorentz_get", 2, comp, v_prev, x, vi);
}

}  // extern "C"
