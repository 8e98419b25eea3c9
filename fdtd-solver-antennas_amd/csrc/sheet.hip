// sheet.hip — conducting sheets: finite-conductivity metal as a surface impedance (include/fdtd_hip_sheet.h).
//
// The implicit part of the sheet's rational admittance is folded into the operator (lumped-edge overrides); what is left is a
// sparse correction of the sheet edges once per timestep, between the E phase and the H update: one thread per edge, plain
// vector loads and stores, state structure-of-arrays.  Every statement is one fp32 operation in the order the header spells
// (-ffp-contract=off), so a host restatement on top of the oracle's half-steps reproduces it bit for bit.
#include "corrections.hpp"
#include "../../include/fdtd_hip_sheet.h"

#include <algorithm>
#include <vector>

namespace {

struct SheetArgs {
  float* V0; float* V1; float* V2;
  const int* off; const int8_t* comp; const float* vi; const int* cls;
  float* vprev; float* ib; const float* alpha; const float* b;
  int n, K;
};

__global__ __launch_bounds__(256) void k_sheet(SheetArgs a) {
  const int e = (int)(blockIdx.x * 256u + threadIdx.x);
  if (e >= a.n) return;
  const int c = a.comp[e];
  float* V = c == 0 ? a.V0 : c == 1 ? a.V1 : a.V2;
  const long o = a.off[e];
  const float* al = a.alpha + (size_t)a.cls[e] * a.K;
  const float* bs = a.b + (size_t)a.cls[e] * a.K;
  float S = 0.0f;
  for (int k = 0; k < a.K; ++k) S = S + al[k] * a.ib[(size_t)k * a.n + e];
  const float v = V[o] - a.vi[e] * S;
  const float avg = 0.5f * (v + a.vprev[e]);
  for (int k = 0; k < a.K; ++k) {
    float* ik = a.ib + (size_t)k * a.n + e;
    *ik = al[k] * *ik + bs[k] * avg;
  }
  V[o] = v;
  a.vprev[e] = v;
}

}  // namespace

// The edge list of a sparse correction (conducting sheets here, lumped elements in lumped.hip)
int edge_list_set(fdtd_ctx* c, EdgeList* l, const CorrectionRow& row, const char* who, int n, const int64_t* idx, const int8_t* comp,
                  const float* vi, const int32_t* cls, int ncls) {
  if (int r = correction_set_state(c, who)) return r;
  const int64_t nn[3] = {c->d.nx, c->d.ny, c->d.nz};
  std::vector<int> off(n), cl(n);
  std::vector<int8_t> cp(n);
  std::vector<int64_t> keys(n);
  for (int e = 0; e < n; ++e) {
    int64_t pos[3];
    if (!sparse_decode(c, idx[e], comp[e], pos, &off[e]) || cls[e] < 0 || cls[e] >= ncls)
      return fdtd_fail(c, FDTD_E_ARG, "%s: edge %d out of range", who, e);
    if (pos[comp[e]] >= nn[comp[e]] - 1) return fdtd_fail(c, FDTD_E_ARG, "%s: edge %d does not exist", who, e);
    keys[e] = idx[e] * 3 + comp[e];
    cp[e] = comp[e];
    cl[e] = cls[e];
  }
  if (sparse_doubles(keys)) return fdtd_fail(c, FDTD_E_ARG, "%s: an edge given twice", who);
  if (int r = correction_set_replace(c, row)) return r;
  if (n == 0) return FDTD_OK;
  hipError_t e = to_device(&l->off, off);
  if (e == hipSuccess) e = to_device(&l->comp, cp);
  if (e == hipSuccess) e = to_device(&l->vi, std::vector<float>(vi, vi + n));
  if (e == hipSuccess) e = to_device(&l->cls, cl);
  if (e == hipSuccess) e = to_device(&l->vprev, std::vector<float>(n, 0.f));
  if (e != hipSuccess) return correction_set_failed(c, row, who, e);
  l->n = n;
  l->facts = edge_facts_of(c, std::move(off));
  return FDTD_OK;
}

void edge_list_free(EdgeList* l) {
  hipFree(l->off); hipFree(l->comp); hipFree(l->vi); hipFree(l->cls); hipFree(l->vprev);
  *l = EdgeList{};
}

namespace {

void sheet_free(fdtd_ctx* c) {
  edge_list_free(&c->sheet);
  hipFree(c->sheet_ib); hipFree(c->sheet_alpha); hipFree(c->sheet_b);
  c->sheet_ib = nullptr; c->sheet_alpha = nullptr; c->sheet_b = nullptr;
  c->sheet_K = c->sheet_ncls = 0;
}

void launch_sheet(fdtd_ctx* c, long long, hipStream_t s) {
  const EdgeList& l = c->sheet;
  if (l.n <= 0) return;
  SheetArgs a{c->p.V[0], c->p.V[1], c->p.V[2], l.off, l.comp, l.vi, l.cls, l.vprev, c->sheet_ib, c->sheet_alpha, c->sheet_b, l.n, c->sheet_K};
  hipLaunchKernelGGL(k_sheet, dim3((unsigned)((l.n + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace

#ifndef __HIP_DEVICE_COMPILE__   // (host data: corrections.hpp)
const CorrectionRow corr_sheet = {
    "conducting sheets", /*no_links*/ false, /*volume*/ false,
    [](const fdtd_ctx* c) { return c->sheet.n > 0; },
    launch_sheet, nullptr, sheet_free,
    [](const fdtd_ctx* c) { return &c->sheet.facts; },
    nullptr};
#endif

extern "C" {

int fdtd_sheet_set(fdtd_ctx* c, int n, const int64_t* idx, const int8_t* comp, const float* vi, const int32_t* cls,
                   int ncls, int K, const float* alpha, const float* b) {
  if (!c) return FDTD_E_ARG;
  if (n < 0 || (n > 0 && (!idx || !comp || !vi || !cls || !alpha || !b)))
    return fdtd_fail(c, FDTD_E_ARG, "fdtd_sheet_set: bad argument");
  if (n > 0 && (K < 1 || K > FDTD_SHEET_MAX_K || ncls < 1))
    return fdtd_fail(c, FDTD_E_ARG, "fdtd_sheet_set: K must be 1..%d and ncls >= 1", FDTD_SHEET_MAX_K);
  if (int r = correction_single_slab(c, corr_sheet)) return r;   // (asked of an empty list as well)
  const int r = edge_list_set(c, &c->sheet, corr_sheet, "fdtd_sheet_set", n, idx, comp, vi, cls, ncls);
  if (r || n == 0) return r;
  hipError_t e = to_device(&c->sheet_ib, std::vector<float>((size_t)K * n, 0.f));
  if (e == hipSuccess) e = to_device(&c->sheet_alpha, std::vector<float>(alpha, alpha + (size_t)ncls * K));
  if (e == hipSuccess) e = to_device(&c->sheet_b, std::vector<float>(b, b + (size_t)ncls * K));
  if (e != hipSuccess) return correction_set_failed(c, corr_sheet, "fdtd_sheet_set", e);
  c->sheet_K = K; c->sheet_ncls = ncls;
  return FDTD_OK;
}

int fdtd_sheet_get(fdtd_ctx* c, float* v_prev, float* i_branch) {
  if (!c) return FDTD_E_ARG;
  HIPCK(c, hipSetDevice(c->d.device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  const int n = c->sheet.n;
  if (n == 0) return FDTD_OK;
  if (v_prev) HIPCK(c, hipMemcpy(v_prev, c->sheet.vprev, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  if (i_branch) HIPCK(c, hipMemcpy(i_branch, c->sheet_ib, (size_t)c->sheet_K * n * sizeof(float), hipMemcpyDeviceToHost));
  return FDTD_OK;
}

}  // extern "C"
