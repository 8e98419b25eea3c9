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
#include "dense_box.hpp"
#include "../../include/fdtd_hip_dispersion.h"

#include <vector>

namespace {

constexpr int TAB = FDTD_DEBYE_MAX_MEDIA * FDTD_DEBYE_MAX_K;   // floats per table (alpha / oma / beta), [medium][MAX_K]

struct DebyeComp {
  float* V;                // the component's voltage array (local plane 0)
  const float* w; const float* vi; const uint8_t* med;
  float* vprev; float* u;
  BoxLaunch l;
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
  unsigned q;
  const DebyeComp& d = box_group(a.c, q);
  if (q >= d.l.nq) return;
  const long of = box_field_offset(d.l, q, a.P, a.plane);         // in the field array
  const size_t o = (size_t)q * 4u;                                // in the box arrays
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
      const float4 t = *reinterpret_cast<const float4*>(d.u + (size_t)k * d.l.n + o);
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
    if (k < K) *reinterpret_cast<float4*>(d.u + (size_t)k * d.l.n + o) = make_float4(ux[k], uy[k], uz[k], uw[k]);
}

}  // namespace

void media_free(MediaBoxes* m) {
  for (auto& b : m->box) { hipFree(b.w); hipFree(b.vi); hipFree(b.vprev); hipFree(b.u); hipFree(b.med); }
  hipFree(m->tab);
  *m = MediaBoxes{};
}

namespace {

void launch_debye(fdtd_ctx* c, long long, hipStream_t s) {
  const MediaBoxes& m = c->debye;
  if (m.nmedia <= 0) return;
  DebyeArgs a{};
  const unsigned blocks = box_layout(c, m.box, a.c);
  if (blocks == 0) return;
  for (int ci = 0; ci < 3; ++ci) {
    const MediaBoxes::Box& b = m.box[ci];
    if (b.g.n == 0) continue;
    DebyeComp& d = a.c[ci];
    d.V = c->p.V[ci]; d.w = b.w; d.vi = b.vi; d.med = b.med; d.vprev = b.vprev; d.u = b.u;
  }
  a.K = m.K; a.P = c->P; a.plane = c->plane; a.tab = m.tab;
  const bool multi = m.nmedia > 1;
  const bool k4 = m.K <= 4;
  auto kern = multi ? (k4 ? k_debye<true, 4> : k_debye<true, 8>) : (k4 ? k_debye<false, 4> : k_debye<false, 8>);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, s, a);
}

}  // namespace

#ifndef __HIP_DEVICE_COMPILE__   // (host data: corrections.hpp)
const CorrectionRow corr_debye = {
    "Debye media", /*no_links*/ true, /*volume*/ true,
    [](const fdtd_ctx* c) { return c->debye.nmedia > 0; },
    launch_debye, nullptr,
    [](fdtd_ctx* c) { media_free(&c->debye); },
    nullptr, nullptr};
#endif

int media_set(fdtd_ctx* c, MediaBoxes* m, const CorrectionRow& row, const char* who, int planes, int nmedia, int K, const std::vector<float>& tab,
              const int32_t lo[3][3], const int32_t hi[3][3], const float* const w[3], const uint8_t* const med[3]) {
  if (int r = correction_set_begin(c, row, who, nmedia > 0)) return r;
  size_t nbox[3] = {0, 0, 0};
  for (int ci = 0; ci < 3 && nmedia > 0; ++ci) {
    if (int r = box_check(c, who, ci, lo[ci], hi[ci], false, "grid's edges", w[ci] && (nmedia == 1 || (med && med[ci])),
                          "weights / medium ids", &nbox[ci]))
      return r;
    if (nmedia > 1)
      for (size_t e = 0; e < nbox[ci]; ++e)
        if (med[ci][e] >= nmedia) return fdtd_fail(c, FDTD_E_ARG, "%s: component %d: medium id %d out of range", who, ci, (int)med[ci][e]);
  }
  if (int r = correction_set_replace(c, row)) return r;
  if (nmedia == 0 || nbox[0] + nbox[1] + nbox[2] == 0) return FDTD_OK;
  std::vector<float> vi;
  if (int r = operator_array(c, 1, &vi)) return r;
  hipError_t e = hipSuccess;
  for (int ci = 0; ci < 3 && e == hipSuccess; ++ci) {
    if (nbox[ci] == 0) continue;
    MediaBoxes::Box& b = m->box[ci];
    b.g = box_widen(lo[ci], hi[ci]);
    std::vector<float> vb(nbox[ci]);
    operator_over_box(c, vi, ci, b.g, vb.data());
    const std::vector<float> vv = scatter(b.g, vb.data());
    std::vector<float> ww = scatter(b.g, w[ci]);
    // an edge the operator holds at zero (vi == 0: a grid face, metal) is no dispersive edge: the correction could never change its
    // voltage, so its states could never act — and on a Mur face the voltage between the two launches is not the timestep's final one
    for (size_t q = 0; q < b.g.n; ++q)
      if (vv[q] == 0.0f) ww[q] = 0.0f;
    e = to_device(&b.w, ww);
    if (e == hipSuccess) e = to_device(&b.vi, vv);
    if (e == hipSuccess && nmedia > 1) e = to_device(&b.med, scatter(b.g, med[ci]));
    if (e == hipSuccess) e = to_device(&b.vprev, std::vector<float>(b.g.n, 0.f));
    if (e == hipSuccess) e = to_device(&b.u, std::vector<float>((size_t)planes * K * b.g.n, 0.f));
  }
  if (e == hipSuccess) e = to_device(&m->tab, tab);
  if (e != hipSuccess) return correction_set_failed(c, row, who, e);
  m->nmedia = nmedia; m->K = K;
  return FDTD_OK;
}

int media_get(fdtd_ctx* c, const MediaBoxes* m, const char* who, int planes, int comp, float* v_prev, float* u, float* vi) {
  if (comp < 0 || comp > 2) return fdtd_fail(c, FDTD_E_ARG, "%s: component %d", who, comp);
  HIPCK(c, hipSetDevice(c->d.device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  const MediaBoxes::Box& b = m->box[comp];
  if (m->nmedia == 0 || b.g.n == 0) return FDTD_OK;
  const size_t nbox = (size_t)(b.g.hi[0] - b.g.lo[0]) * (b.g.hi[1] - b.g.lo[1]) * (b.g.hi[2] - b.g.lo[2]);
  if (v_prev) HIPCK(c, crop(b.g, b.vprev, v_prev));
  if (vi) HIPCK(c, crop(b.g, b.vi, vi));
  if (u)
    for (int p = 0; p < planes * m->K; ++p) HIPCK(c, crop(b.g, b.u + (size_t)p * b.g.n, u + (size_t)p * nbox));
  return FDTD_OK;
}

extern "C" {

int fdtd_debye_set(fdtd_ctx* c, int nmedia, int K, const float* alpha, const float* oma, const float* beta,
                   const int32_t lo[3][3], const int32_t hi[3][3], const float* const w[3], const uint8_t* const med[3]) {
  if (!c) return FDTD_E_ARG;
  if (nmedia < 0 || nmedia > FDTD_DEBYE_MAX_MEDIA)
    return fdtd_fail(c, FDTD_E_ARG, "fdtd_debye_set: at most %d media", FDTD_DEBYE_MAX_MEDIA);
  if (nmedia > 0 && (K < 1 || K > FDTD_DEBYE_MAX_K)) return fdtd_fail(c, FDTD_E_ARG, "fdtd_debye_set: K must be 1..%d", FDTD_DEBYE_MAX_K);
  if (nmedia > 0 && (!alpha || !oma || !beta || !lo || !hi || !w)) return fdtd_fail(c, FDTD_E_ARG, "fdtd_debye_set: bad argument");
  std::vector<float> tab(3 * TAB, 0.f);
  const float* src[3] = {alpha, oma, beta};
  for (int t = 0; t < 3; ++t)
    for (int m = 0; m < nmedia; ++m)
      for (int k = 0; k < K; ++k) tab[(size_t)t * TAB + m * FDTD_DEBYE_MAX_K + k] = src[t][m * K + k];
  return media_set(c, &c->debye, corr_debye, "fdtd_debye_set", 1, nmedia, K, tab, lo, hi, w, med);
}

int fdtd_debye_get(fdtd_ctx* c, int comp, float* v_prev, float* u, float* vi) {
  if (!c) return FDTD_E_ARG;
  return media_get(c, &c->debye, "fdtd_debye_get", 1, comp, v_prev, u, vi);
}

}  // extern "C"
