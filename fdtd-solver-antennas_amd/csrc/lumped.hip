// lumped.hip — lumped R-L-C elements on mesh edges (include/fdtd_hip_lumped.h).
//
// The implicit part of the element's trapezoidal branch is folded into the operator (lumped-edge overrides); what is left is a
// sparse correction of the element edges once per timestep, between the E phase and the H update, after the corrections of the
// Debye media and the conducting sheets: one thread per edge, plain vector loads and stores, the two states structure-of-arrays.
// The edges are few (one to a few thousand): the launch is a latency floor, not a bandwidth problem.  Every statement is one
// fp32 operation in the order the header spells (-ffp-contract=off), so a host restatement on top of the oracle's half-steps
// reproduces it bit for bit.
#include "fdtd_ctx.h"
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

}  // namespace

void lumped_free(fdtd_ctx* c) {
  hipFree(c->lumped_off); hipFree(c->lumped_comp); hipFree(c->lumped_vi); hipFree(c->lumped_cls);
  hipFree(c->lumped_vprev); hipFree(c->lumped_x); hipFree(c->lumped_phi); hipFree(c->lumped_gam); hipFree(c->lumped_h);
  c->lumped_off = nullptr; c->lumped_comp = nullptr; c->lumped_vi = nullptr; c->lumped_cls = nullptr;
  c->lumped_vprev = nullptr; c->lumped_x = nullptr; c->lumped_phi = nullptr; c->lumped_gam = nullptr; c->lumped_h = nullptr;
  c->lumped_n = 0;
  c->h_lumped_off.clear();
  c->lumped_faces = 0;
}

void launch_lumped(fdtd_ctx* c, hipStream_t s) {
  if (c->lumped_n <= 0) return;
  LumpedArgs a{c->p.V[0], c->p.V[1], c->p.V[2], c->lumped_off, c->lumped_comp, c->lumped_vi, c->lumped_cls,
               c->lumped_vprev, c->lumped_x, c->lumped_phi, c->lumped_gam, c->lumped_h, c->lumped_n};
  hipLaunchKernelGGL(k_lumped, dim3((unsigned)((c->lumped_n + 255) / 256)), dim3(256), 0, s, a);
}

extern "C" {

int fdtd_lumped_set(fdtd_ctx* c, int n, const int64_t* idx, const int8_t* comp, const float* vi, const int32_t* cls, int ncls,
                    const float* phi, const float* gam, const float* h) {
  if (!c) return FDTD_E_ARG;
  if (n < 0 || (n > 0 && (!idx || !comp || !vi || !cls || !phi || !gam || !h)))
    return fdtd_fail(c, FDTD_E_ARG, "fdtd_lumped_set: bad argument");
  if (n > 0 && ncls < 1) return fdtd_fail(c, FDTD_E_ARG, "fdtd_lumped_set: ncls must be >= 1");
  if (c->d.world > 1) return fdtd_fail(c, FDTD_E_UNSUPPORTED, "lumped elements: single slab only (world = 1)");
  if (!c->have_op) return fdtd_fail(c, FDTD_E_STATE, "fdtd_lumped_set: set the operator first");
  if (c->step != 0) return fdtd_fail(c, FDTD_E_STATE, "fdtd_lumped_set: before the first timestep");
  std::vector<int> off, cl;
  std::vector<int8_t> cp;
  unsigned faces = 0;
  if (int r = sparse_edges_check(c, "fdtd_lumped_set", n, idx, comp, cls, ncls, &off, &cp, &cl, &faces)) return r;
  std::vector<float> v(vi, vi + n);
  HIPCK(c, hipSetDevice(c->d.device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  lumped_free(c);
  if (n == 0) return FDTD_OK;
  std::vector<float> ph(phi, phi + (size_t)ncls * 4), gm(gam, gam + (size_t)ncls * 2), hh(h, h + (size_t)ncls * 2);
  std::vector<float> zero((size_t)2 * n, 0.f);
  hipError_t e = sparse_upload(&c->lumped_off, off);
  if (e == hipSuccess) e = sparse_upload(&c->lumped_comp, cp);
  if (e == hipSuccess) e = sparse_upload(&c->lumped_vi, v);
  if (e == hipSuccess) e = sparse_upload(&c->lumped_cls, cl);
  if (e == hipSuccess) e = sparse_upload(&c->lumped_vprev, std::vector<float>(zero.begin(), zero.begin() + n));
  if (e == hipSuccess) e = sparse_upload(&c->lumped_x, zero);
  if (e == hipSuccess) e = sparse_upload(&c->lumped_phi, ph);
  if (e == hipSuccess) e = sparse_upload(&c->lumped_gam, gm);
  if (e == hipSuccess) e = sparse_upload(&c->lumped_h, hh);
  if (e != hipSuccess) {
    lumped_free(c);
    return fdtd_fail(c, e == hipErrorOutOfMemory ? FDTD_E_NOMEM : FDTD_E_DEVICE, "fdtd_lumped_set: %s", hipGetErrorString(e));
  }
  c->lumped_n = n;
  // what the planner asks (api.hip: correction_on_face, correction_at): the faces the edges touch, their offsets for the V-probes
  c->lumped_faces = faces;
  c->h_lumped_off = off;
  std::sort(c->h_lumped_off.begin(), c->h_lumped_off.end());
  return FDTD_OK;
}

int fdtd_lumped_get(fdtd_ctx* c, float* v_prev, float* x) {
  if (!c) return FDTD_E_ARG;
  HIPCK(c, hipSetDevice(c->d.device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  if (c->lumped_n == 0) return FDTD_OK;
  if (v_prev) HIPCK(c, hipMemcpy(v_prev, c->lumped_vprev, (size_t)c->lumped_n * sizeof(float), hipMemcpyDeviceToHost));
  if (x) HIPCK(c, hipMemcpy(x, c->lumped_x, (size_t)2 * c->lumped_n * sizeof(float), hipMemcpyDeviceToHost));
  return FDTD_OK;
}

}  // extern "C"
