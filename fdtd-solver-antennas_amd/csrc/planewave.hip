// planewave.hip — plane-wave excitation on a total-field / scattered-field box (include/fdtd_hip_planewave.h).
//
// The update kernels stay what they are: they difference total against scattered fields across the box surface, and two sparse
// corrections per timestep add the analytic incident field each of those differences missed — to the tangential edges on the box
// surface after the E phase, to the faces just outside it after the H update.  Both lists are SURFACE sets (a few 10^4 entries at
// most), so k_planewave is a latency floor like k_lumped and k_conformal: one thread per entry, the entry's arrays read from
// consecutive memory by consecutive lanes, the pulse table (a few thousand floats, shared by all lanes) through L1, one scattered
// load and store of the field.  No state, no atomics: the host merges the two terms of an element on a box edge into ONE entry, so
// no element is written twice in a launch.  Every statement is one fp32 operation in the order the header spells
// (-ffp-contract=off), so a host restatement on top of the oracle's half-steps reproduces it bit for bit.
#include "corrections.hpp"
#include "../../include/fdtd_hip_planewave.h"

#include <algorithm>
#include <vector>

namespace {

struct PlaneWaveArgs {
  float* F0; float* F1; float* F2;
  const int* off; const int8_t* comp; const float2* coef; const int2* m0; const float2* w;
  const float* sig2;
  long long base;   // 2 n - 1 (E list) or 2 n (H list)
  int nsig2, n;
};

// sig2 taken as zero outside the table
__device__ __forceinline__ float pw_sig(const float* __restrict__ sig2, const int nsig2, const long long p) {
  return (p >= 0 && p < (long long)nsig2) ? sig2[p] : 0.f;
}
__device__ __forceinline__ float pw_term(const float* __restrict__ sig2, const int nsig2, const long long p, const float w, const float coef) {
  const float hi = pw_sig(sig2, nsig2, p);
  const float a = pw_sig(sig2, nsig2, p - 1) - hi;
  const float b = w * a;
  const float s = hi + b;
  return coef * s;
}

__global__ __launch_bounds__(256) void k_planewave(const PlaneWaveArgs a) {
  const int e = (int)(blockIdx.x * 256u + threadIdx.x);
  if (e >= a.n) return;
  const int c = a.comp[e];
  float* F = c == 0 ? a.F0 : c == 1 ? a.F1 : a.F2;
  const long o = a.off[e];
  const float2 cf = a.coef[e];
  const int2 m = a.m0[e];
  const float2 w = a.w[e];
  const float t0 = pw_term(a.sig2, a.nsig2, a.base - m.x, w.x, cf.x);
  const float t1 = pw_term(a.sig2, a.nsig2, a.base - m.y, w.y, cf.y);
  const float g = F[o] + t0;
  F[o] = g + t1;
}

void list_free(fdtd_ctx::PlaneWaveList* l) {
  hipFree(l->off); hipFree(l->comp); hipFree(l->coef); hipFree(l->m0); hipFree(l->w);
  *l = fdtd_ctx::PlaneWaveList{};
}

// one list checked and turned into the arrays the kernel reads (nothing on the device yet)
struct HostList { std::vector<int> off; std::vector<int8_t> comp; std::vector<float2> coef, w; std::vector<int2> m0; };
int list_check(fdtd_ctx* c, const char* what, bool faces, int n, const int64_t* idx, const int8_t* comp, const float* coef,
               const int32_t* m0, const float* w, HostList* out) {
  const int64_t nn[3] = {c->d.nx, c->d.ny, c->d.nz};
  std::vector<int64_t> keys((size_t)n);
  out->off.resize(n); out->comp.resize(n); out->coef.resize(n); out->w.resize(n); out->m0.resize(n);
  for (int e = 0; e < n; ++e) {
    const int m = comp[e];
    int64_t pos[3];
    int off;
    if (!sparse_decode(c, idx[e], m, pos, &off)) return fdtd_fail(c, FDTD_E_ARG, "fdtd_planewave_set: %s %d out of range", what, e);
    // an edge spans one cell along its own axis, a face one cell along both transverse axes
    const bool exists = faces ? (pos[(m + 1) % 3] < nn[(m + 1) % 3] - 1 && pos[(m + 2) % 3] < nn[(m + 2) % 3] - 1) : pos[m] < nn[m] - 1;
    if (!exists) return fdtd_fail(c, FDTD_E_ARG, "fdtd_planewave_set: %s %d does not exist", what, e);
    for (int q = 0; q < 2; ++q) {
      if (m0[2 * (size_t)e + q] < 0) return fdtd_fail(c, FDTD_E_ARG, "fdtd_planewave_set: %s %d has a negative delay", what, e);
      const float wq = w[2 * (size_t)e + q];
      if (!(wq >= 0.f && wq < 1.f)) return fdtd_fail(c, FDTD_E_ARG, "fdtd_planewave_set: %s %d: the fraction of the delay must be in [0, 1)", what, e);
    }
    keys[e] = idx[e] * 3 + m;
    out->off[e] = off; out->comp[e] = (int8_t)m;
    out->coef[e] = make_float2(coef[2 * (size_t)e], coef[2 * (size_t)e + 1]);
    out->m0[e] = make_int2(m0[2 * (size_t)e], m0[2 * (size_t)e + 1]);
    out->w[e] = make_float2(w[2 * (size_t)e], w[2 * (size_t)e + 1]);
  }
  if (sparse_doubles(keys)) return fdtd_fail(c, FDTD_E_ARG, "fdtd_planewave_set: %s given twice", faces ? "a face" : "an edge");
  return FDTD_OK;
}
hipError_t list_upload(fdtd_ctx::PlaneWaveList* l, const HostList& h) {
  hipError_t e = to_device(&l->off, h.off);
  if (e == hipSuccess) e = to_device(&l->comp, h.comp);
  if (e == hipSuccess) e = to_device(&l->coef, h.coef);
  if (e == hipSuccess) e = to_device(&l->m0, h.m0);
  if (e == hipSuccess) e = to_device(&l->w, h.w);
  if (e == hipSuccess) l->n = (int)h.off.size();
  return e;
}

void planewave_free(fdtd_ctx* c) {
  list_free(&c->pw[0]); list_free(&c->pw[1]);
  hipFree(c->pw_sig2); c->pw_sig2 = nullptr; c->pw_nsig2 = 0;
}

void launch_planewave(fdtd_ctx* c, int kind, long long step, hipStream_t s) {
  const fdtd_ctx::PlaneWaveList& l = c->pw[kind == FDTD_KIND_V ? 0 : 1];
  if (l.n <= 0) return;
  float* const* F = kind == FDTD_KIND_V ? c->p.V : c->p.I;
  PlaneWaveArgs a{F[0], F[1], F[2], l.off, l.comp, l.coef, l.m0, l.w, c->pw_sig2, 2 * step - (kind == FDTD_KIND_V ? 1 : 0), c->pw_nsig2, l.n};
  hipLaunchKernelGGL(k_planewave, dim3((unsigned)((l.n + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace

#ifndef __HIP_DEVICE_COMPILE__   // (host data: corrections.hpp)
// (the one correction of both sides: its edge list runs behind the E phase, its face list behind the H update)
const CorrectionRow corr_planewave = {
    "plane-wave excitation", /*no_links*/ true, /*volume*/ false,
    [](const fdtd_ctx* c) { return c->pw[0].n > 0 || c->pw[1].n > 0; },
    [](fdtd_ctx* c, long long step, hipStream_t s) { launch_planewave(c, FDTD_KIND_V, step, s); },
    [](fdtd_ctx* c, long long step, hipStream_t s) { launch_planewave(c, FDTD_KIND_I, step, s); },
    planewave_free,
    [](const fdtd_ctx* c) { return &c->pw[0].facts; },
    nullptr};
#endif

extern "C" {

int fdtd_planewave_set(fdtd_ctx* c,
                       int nE, const int64_t* idxE, const int8_t* compE, const float* coefE, const int32_t* m0E, const float* wE,
                       int nH, const int64_t* idxH, const int8_t* compH, const float* coefH, const int32_t* m0H, const float* wH,
                       const float* sig2, int nsig2) {
  if (!c) return FDTD_E_ARG;
  if (nE < 0 || nH < 0 || (nE > 0 && (!idxE || !compE || !coefE || !m0E || !wE)) || (nH > 0 && (!idxH || !compH || !coefH || !m0H || !wH)) ||
      ((nE > 0 || nH > 0) && (!sig2 || nsig2 < 1)))
    return fdtd_fail(c, FDTD_E_ARG, "fdtd_planewave_set: bad argument");
  if (int r = correction_set_begin(c, corr_planewave, "fdtd_planewave_set", nE > 0 || nH > 0)) return r;
  HostList hE, hH;
  if (int r = list_check(c, "edge", false, nE, idxE, compE, coefE, m0E, wE, &hE)) return r;
  if (int r = list_check(c, "face", true, nH, idxH, compH, coefH, m0H, wH, &hH)) return r;
  if (int r = correction_set_replace(c, corr_planewave)) return r;
  if (nE == 0 && nH == 0) return FDTD_OK;
  hipError_t e = list_upload(&c->pw[0], hE);
  if (e == hipSuccess) e = list_upload(&c->pw[1], hH);
  if (e == hipSuccess) e = to_device(&c->pw_sig2, std::vector<float>(sig2, sig2 + nsig2));
  if (e != hipSuccess) return correction_set_failed(c, corr_planewave, "fdtd_planewave_set", e);
  c->pw_nsig2 = nsig2;
  // what the planner asks of the edge list (api.hip correction_on_face, correction_at): a V-probe cell on a listed edge is sampled in
  // front of the corrections, a listed edge on the node plane of a Mur face takes the apply pass as a launch of its own
  c->pw[0].facts = edge_facts_of(c, std::move(hE.off));
  return FDTD_OK;
}

}  // extern "C"
