// sheet.hip — conducting sheets: finite-conductivity metal as a surface impedance (include/fdtd_hip_sheet.h).
//
// The implicit part of the sheet's rational admittance is folded into the operator (lumped-edge overrides); what is left is a
// sparse correction of the sheet edges once per timestep, between the E phase and the H update: one thread per edge, plain
// vector loads and stores, state structure-of-arrays.  Every statement is one fp32 operation in the order the header spells
// (-ffp-contract=off), so a host restatement on top of the oracle's half-steps reproduces it bit for bit.
#include "fdtd_ctx.h"
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

// The edge list of a sparse correction (conducting sheets here, lumped elements in lumped.hip): every edge inside the grid and
// existing, classes in range, no edge twice.  Out: local offsets, components and classes as the kernels take them, and the grid
// faces whose node plane holds an edge (bit f: x-, x+, y-, y+, z-, z+) — what the planner asks (api.hip).
int sparse_edges_check(fdtd_ctx* c, const char* who, int n, const int64_t* idx, const int8_t* comp, const int32_t* cls, int ncls,
                       std::vector<int>* off_out, std::vector<int8_t>* comp_out, std::vector<int>* cls_out, unsigned* faces_out) {
  const int64_t gplane = (int64_t)c->d.nx * c->d.ny;
  const int64_t nn[3] = {c->d.nx, c->d.ny, c->d.nz};
  std::vector<int> off(n), cl(n);
  std::vector<int8_t> cp(n);
  std::vector<int64_t> keys(n);
  unsigned faces = 0;
  for (int e = 0; e < n; ++e) {
    const int64_t g = idx[e];
    if (g < 0 || g >= gplane * c->d.nz || comp[e] < 0 || comp[e] > 2 || cls[e] < 0 || cls[e] >= ncls)
      return fdtd_fail(c, FDTD_E_ARG, "%s: edge %d out of range", who, e);
    const int64_t k = g / gplane, r = g - k * gplane, j = r / c->d.nx, i = r - j * c->d.nx;
    const int64_t pos[3] = {i, j, k};
    if (pos[comp[e]] >= nn[comp[e]] - 1) return fdtd_fail(c, FDTD_E_ARG, "%s: edge %d does not exist", who, e);
    keys[e] = g * 3 + comp[e];
    for (int a = 0; a < 3; ++a) faces |= (pos[a] == 0 ? 1u : 0u) << (2 * a) | (pos[a] == nn[a] - 1 ? 1u : 0u) << (2 * a + 1);
    off[e] = (int)((k - c->d.k0) * c->plane + j * c->P + i);
    cp[e] = comp[e];
    cl[e] = cls[e];
  }
  std::sort(keys.begin(), keys.end());
  if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) return fdtd_fail(c, FDTD_E_ARG, "%s: an edge given twice", who);
  off_out->swap(off); comp_out->swap(cp); cls_out->swap(cl);
  *faces_out = faces;
  return FDTD_OK;
}

void sheet_free(fdtd_ctx* c) {
  hipFree(c->sheet_off); hipFree(c->sheet_comp); hipFree(c->sheet_vi); hipFree(c->sheet_cls);
  hipFree(c->sheet_vprev); hipFree(c->sheet_ib); hipFree(c->sheet_alpha); hipFree(c->sheet_b);
  c->sheet_off = nullptr; c->sheet_comp = nullptr; c->sheet_vi = nullptr; c->sheet_cls = nullptr;
  c->sheet_vprev = nullptr; c->sheet_ib = nullptr; c->sheet_alpha = nullptr; c->sheet_b = nullptr;
  c->sheet_n = c->sheet_K = c->sheet_ncls = 0;
  c->h_sheet_off.clear();
  c->sheet_faces = 0;
}

void launch_sheet(fdtd_ctx* c, hipStream_t s) {
  if (c->sheet_n <= 0) return;
  SheetArgs a{c->p.V[0], c->p.V[1], c->p.V[2], c->sheet_off, c->sheet_comp, c->sheet_vi, c->sheet_cls,
              c->sheet_vprev, c->sheet_ib, c->sheet_alpha, c->sheet_b, c->sheet_n, c->sheet_K};
  hipLaunchKernelGGL(k_sheet, dim3((unsigned)((c->sheet_n + 255) / 256)), dim3(256), 0, s, a);
}

extern "C" {

int fdtd_sheet_set(fdtd_ctx* c, int n, const int64_t* idx, const int8_t* comp, const float* vi, const int32_t* cls,
                   int ncls, int K, const float* alpha, const float* b) {
  if (!c) return FDTD_E_ARG;
  if (n < 0 || (n > 0 && (!idx || !comp || !vi || !cls || !alpha || !b)))
    return fdtd_fail(c, FDTD_E_ARG, "fdtd_sheet_set: bad argument");
  if (n > 0 && (K < 1 || K > FDTD_SHEET_MAX_K || ncls < 1))
    return fdtd_fail(c, FDTD_E_ARG, "fdtd_sheet_set: K must be 1..%d and ncls >= 1", FDTD_SHEET_MAX_K);
  if (c->d.world > 1) return fdtd_fail(c, FDTD_E_UNSUPPORTED, "conducting sheets: single slab only (world = 1)");
  if (!c->have_op) return fdtd_fail(c, FDTD_E_STATE, "fdtd_sheet_set: set the operator first");
  if (c->step != 0) return fdtd_fail(c, FDTD_E_STATE, "fdtd_sheet_set: before the first timestep");
  std::vector<int> off, cl;
  std::vector<int8_t> cp;
  unsigned faces = 0;
  if (int r = sparse_edges_check(c, "fdtd_sheet_set", n, idx, comp, cls, ncls, &off, &cp, &cl, &faces)) return r;
  std::vector<float> v(vi, vi + n);
  HIPCK(c, hipSetDevice(c->d.device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  sheet_free(c);
  if (n == 0) return FDTD_OK;
  std::vector<float> al(alpha, alpha + (size_t)ncls * K), bb(b, b + (size_t)ncls * K);
  std::vector<float> zero((size_t)K * n, 0.f);
  hipError_t e = sparse_upload(&c->sheet_off, off);
  if (e == hipSuccess) e = sparse_upload(&c->sheet_comp, cp);
  if (e == hipSuccess) e = sparse_upload(&c->sheet_vi, v);
  if (e == hipSuccess) e = sparse_upload(&c->sheet_cls, cl);
  if (e == hipSuccess) e = sparse_upload(&c->sheet_vprev, std::vector<float>(zero.begin(), zero.begin() + n));
  if (e == hipSuccess) e = sparse_upload(&c->sheet_ib, zero);
  if (e == hipSuccess) e = sparse_upload(&c->sheet_alpha, al);
  if (e == hipSuccess) e = sparse_upload(&c->sheet_b, bb);
  if (e != hipSuccess) {
    sheet_free(c);
    return fdtd_fail(c, e == hipErrorOutOfMemory ? FDTD_E_NOMEM : FDTD_E_DEVICE, "fdtd_sheet_set: %s", hipGetErrorString(e));
  }
  c->sheet_n = n; c->sheet_K = K; c->sheet_ncls = ncls;
  // what the planner asks (api.hip: mur_direct_possible, probes_first): the faces the edges touch, their offsets for the V-probes
  c->sheet_faces = faces;
  c->h_sheet_off = off;
  std::sort(c->h_sheet_off.begin(), c->h_sheet_off.end());
  return FDTD_OK;
}

int fdtd_sheet_get(fdtd_ctx* c, float* v_prev, float* i_branch) {
  if (!c) return FDTD_E_ARG;
  HIPCK(c, hipSetDevice(c->d.device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  if (c->sheet_n == 0) return FDTD_OK;
  if (v_prev) HIPCK(c, hipMemcpy(v_prev, c->sheet_vprev, (size_t)c->sheet_n * sizeof(float), hipMemcpyDeviceToHost));
  if (i_branch) HIPCK(c, hipMemcpy(i_branch, c->sheet_ib, (size_t)c->sheet_K * c->sheet_n * sizeof(float), hipMemcpyDeviceToHost));
  return FDTD_OK;
}

}  // extern "C"
