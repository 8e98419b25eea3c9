// lumped.hip — lumped R-L-C elements on mesh edges (include/fdtd_hip_lumped.h).
//
// The implicit part of the element's trapezoidal branch is folded into the operator (lumped-edge overrides); what is left is a
// sparse correction of the element edges once per timestep, between the E phase and the H update, after the corrections of the
// Debye media and the conducting sheets: one thread per edge, plain vector loads and stores, the two states structure-of-arrays.
// The edges are few (one to a few thousand): the launch is a latency floor, not a bandwidth problem.  Every statement is one
// fp32 operation in the order the header spells (-ffp-contract=off), so a host restatement on top of the oracle's half-steps
// reproduces it bit for bit.
#include "corrections.hpp"
#include "../../include/fdtd_hip_lumped.h"

#include <algorithm>
#include <vector>

namespace {

struct LumpedArgs {
  float* V0; float* V1; float* V2;
  const int* off; const int8_t* comp; const float* vi; const int* cls;
  float* vprev; float* x; const float* phi; const float* gam; const float* h;
  int n;
};

__global__ __launch_bounds__(256) void k_lumped(LumpedArgs a) {
  const int e = (int)(blockIdx.x * 256u + threadIdx.x);
  if (e >= a.n) return;
  const int c = a.comp[e];
  float* V = c == 0 ? a.V0 : c == 1 ? a.V1 : a.V2;
  const long o = a.off[e];
  const float* ph = a.phi + (size_t)a.cls[e] * 4;
  const float* gm = a.gam + (size_t)a.cls[e] * 2;
  const float* hh = a.h + (size_t)a.cls[e] * 2;
  const float x0 = a.x[e], x1 = a.x[(size_t)a.n + e];
  const float S = hh[0] * x0 + hh[1] * x1;
  const float v = V[o] - a.vi[e] * S;
  const float avg = 0.5f * (v + a.vprev[e]);
  a.x[e] = (ph[0] * x0 + ph[1] * x1) + gm[0] * avg;
  a.x[(size_t)a.n + e] = (ph[2] * x0 + ph[3] * x1) + gm[1] * avg;
  V[o] = v;
  a.vprev[e] = v;
}

void lumped_free(fdtd_ctx* c) {
  edge_list_free(&c->lumped);
  hipFree(c->lumped_x); hipFree(c->lumped_phi); hipFree(c->lumped_gam); hipFree(c->lumped_h);
  c->lumped_x = nullptr; c->lumped_phi = nullptr; c->lumped_gam = nullptr; c->lumped_h = nullptr;
}

void launch_lumped(fdtd_ctx* c, long long, hipStream_t s) {
  const EdgeList& l = c->lumped;
  if (l.n <= 0) return;
  LumpedArgs a{c->p.V[0], c->p.V[1], c->p.V[2], l.off, l.comp, l.vi, l.cls, l.vprev, c->lumped_x, c->lumped_phi, c->lumped_gam, c->lumped_h, l.n};
  hipLaunchKernelGGL(k_lumped, dim3((unsigned)((l.n + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace

#ifndef __HIP_DEVICE_COMPILE__   // (host data: corrections.hpp)
const CorrectionRow corr_lumped = {
    "lumped elements", /*no_links*/ true, /*volume*/ false,
    [](const fdtd_ctx* c) { return c->lumped.n > 0; },
    launch_lumped, nullptr, lumped_free,
    [](const fdtd_ctx* c) { return &c->lumped.facts; },
    nullptr};
#endif

extern "C" {

int fdtd_lumped_set(fdtd_ctx* c, int n, const int64_t* idx, const int8_t* comp, const float* vi, const int32_t* cls, int ncls,
                    const float* phi, const float* gam, const float* h) {
  if (!c) return FDTD_E_ARG;
  if (n < 0 || (n > 0 && (!idx || !comp || !vi || !cls || !phi || !gam || !h)))
    return fdtd_fail(c, FDTD_E_ARG, "fdtd_lumped_set: bad argument");
  if (n > 0 && ncls < 1) return fdtd_fail(c, FDTD_E_ARG, "fdtd_lumped_set: ncls must be >= 1");
  // (this call's own wording; the planner refuses p2p and linked contexts when they step: api.hip plan_schedule)
  if (c->d.world > 1) return fdtd_fail(c, FDTD_E_UNSUPPORTED, "lumped elements: single slab only (world = 1)");
  const int r = edge_list_set(c, &c->lumped, corr_lumped, "fdtd_lumped_set", n, idx, comp, vi, cls, ncls);
  if (r || n == 0) return r;
  hipError_t e = to_device(&c->lumped_x, std::vector<float>((size_t)2 * n, 0.f));
  if (e == hipSuccess) e = to_device(&c->lumped_phi, std::vector<float>(phi, phi + (size_t)ncls * 4));
  if (e == hipSuccess) e = to_device(&c->lumped_gam, std::vector<float>(gam, gam + (size_t)ncls * 2));
  if (e == hipSuccess) e = to_device(&c->lumped_h, std::vector<float>(h, h + (size_t)ncls * 2));
  if (e != hipSuccess) return correction_set_failed(c, corr_lumped, "fdtd_lumped_set", e);
  return FDTD_OK;
}

int fdtd_lumped_get(fdtd_ctx* c, float* v_prev, float* x) {
  if (!c) return FDTD_E_ARG;
  HIPCK(c, hipSetDevice(c->d.device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  const int n = c->lumped.n;
  if (n == 0) return FDTD_OK;
  if (v_prev) HIPCK(c, hipMemcpy(v_prev, c->lumped.vprev, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  if (x) HIPCK(c, hipMemcpy(x, c->lumped_x, (size_t)2 * n * sizeof(float), hipMemcpyDeviceToHost));
  return FDTD_OK;
}

}  // extern "C"
