// conformal.hip — conformal (Dey-Mittra) PEC boundaries (include/fdtd_hip_conformal.h).
//
// The operator and the H kernels stay what they are; a face the metal surface cuts needs I <- i_prev + sum+- coef_e V_e with its own
// four coefficients (iv0 f_e / a_f), restored by a correction after the H update of every timestep.  The cut faces are a SURFACE
// effect, a few thousand faces on a grid of millions, so the correction is sparse: one thread per listed face, its record (offset,
// component, four coefficients: 32 bytes, two 16-byte loads) and i_prev read from consecutive memory by consecutive lanes, four
// gathered voltages, one scattered current.  Every statement is one fp32 operation in the order the header spells
// (-ffp-contract=off), so a host restatement on top of the oracle's half-steps reproduces it bit for bit.
#include "corrections.hpp"
#include "../../include/fdtd_hip_conformal.h"

#include <algorithm>
#include <vector>

namespace {

struct ConfArgs {
  const float* V0; const float* V1; const float* V2;
  float* I0; float* I1; float* I2;
  const int4* face;        // x: offset of the face's node, y: component, z, w: unused
  const float4* coef;
  float* iprev;
  int n, P, plane;
};

__global__ __launch_bounds__(256) void k_conformal(const ConfArgs a) {
  const int f = (int)(blockIdx.x * 256u + threadIdx.x);
  if (f >= a.n) return;
  const int4 fc = a.face[f];
  const float4 cf = a.coef[f];
  const int n = fc.y;
  const long o = fc.x;
  // a1 = (n + 1) % 3, a2 = (n + 2) % 3: the voltages along a2 differenced along a1, those along a1 differenced along a2
  const float* Va2 = n == 0 ? a.V2 : n == 1 ? a.V0 : a.V1;
  const float* Va1 = n == 0 ? a.V1 : n == 1 ? a.V2 : a.V0;
  const long s1 = n == 0 ? a.P : n == 1 ? a.plane : 1;
  const long s2 = n == 0 ? a.plane : n == 1 ? 1 : a.P;
  float* I = n == 0 ? a.I0 : n == 1 ? a.I1 : a.I2;
  const float t0 = cf.x * Va2[o];
  const float t1 = cf.y * Va2[o + s1];
  const float t2 = cf.z * Va1[o];
  const float t3 = cf.w * Va1[o + s2];
  const float d1 = t0 - t1;
  const float d2 = t2 - t3;
  const float s = d1 - d2;
  const float r = a.iprev[f] + s;
  I[o] = r;
  a.iprev[f] = r;
}

// i_prev <- I of the listed faces (of one component; comp < 0: of all)
__global__ __launch_bounds__(256) void k_conformal_prime(const ConfArgs a, const int comp) {
  const int f = (int)(blockIdx.x * 256u + threadIdx.x);
  if (f >= a.n) return;
  const int4 fc = a.face[f];
  if (comp >= 0 && fc.y != comp) return;
  const float* I = fc.y == 0 ? a.I0 : fc.y == 1 ? a.I1 : a.I2;
  a.iprev[f] = I[fc.x];
}

ConfArgs conf_args(fdtd_ctx* c) {
  return ConfArgs{c->p.V[0], c->p.V[1], c->p.V[2], c->p.I[0], c->p.I[1], c->p.I[2], c->conf_face, c->conf_coef, c->conf_iprev,
                  c->conf_n, c->P, c->plane};
}

void conformal_free(fdtd_ctx* c) {
  hipFree(c->conf_face); hipFree(c->conf_coef); hipFree(c->conf_iprev);
  c->conf_face = nullptr; c->conf_coef = nullptr; c->conf_iprev = nullptr;
  c->conf_n = 0;
}

void launch_conformal(fdtd_ctx* c, long long, hipStream_t s) {
  if (c->conf_n <= 0) return;
  hipLaunchKernelGGL(k_conformal, dim3((unsigned)((c->conf_n + 255) / 256)), dim3(256), 0, s, conf_args(c));
}

int conformal_prime(fdtd_ctx* c, int comp) {
  if (c->conf_n <= 0) return FDTD_OK;
  hipLaunchKernelGGL(k_conformal_prime, dim3((unsigned)((c->conf_n + 255) / 256)), dim3(256), 0, c->stream, conf_args(c), comp);
  HIPCK(c, hipGetLastError());
  HIPCK(c, hipStreamSynchronize(c->stream));
  return FDTD_OK;
}

}  // namespace

#ifndef __HIP_DEVICE_COMPILE__   // (host data: corrections.hpp)
const CorrectionRow corr_conformal = {
    "conformal boundaries", /*no_links*/ true, /*volume*/ false,
    [](const fdtd_ctx* c) { return c->conf_n > 0; },
    nullptr, launch_conformal, conformal_free, nullptr, conformal_prime};
#endif

extern "C" {

int fdtd_conformal_set(fdtd_ctx* c, int n, const int8_t* comp, const int64_t* idx, const float* coef) {
  if (!c) return FDTD_E_ARG;
  if (n < 0 || (n > 0 && (!comp || !idx || !coef))) return fdtd_fail(c, FDTD_E_ARG, "fdtd_conformal_set: bad argument");
  if (int r = correction_set_begin(c, corr_conformal, "fdtd_conformal_set", n > 0)) return r;
  const int64_t nn[3] = {c->d.nx, c->d.ny, c->d.nz};
  std::vector<int4> face((size_t)n);
  std::vector<float4> cf((size_t)n);
  std::vector<int64_t> keys((size_t)n);
  for (int f = 0; f < n; ++f) {
    const int m = comp[f];
    int64_t pos[3];
    int off;
    if (!sparse_decode(c, idx[f], m, pos, &off)) return fdtd_fail(c, FDTD_E_ARG, "fdtd_conformal_set: face %d out of range", f);
    // the face spans one cell along both transverse axes: its four edges reach the nodes p + e_a1 and p + e_a2
    if (pos[(m + 1) % 3] >= nn[(m + 1) % 3] - 1 || pos[(m + 2) % 3] >= nn[(m + 2) % 3] - 1)
      return fdtd_fail(c, FDTD_E_ARG, "fdtd_conformal_set: face %d does not exist", f);
    keys[f] = idx[f] * 3 + m;
    face[f] = make_int4(off, m, 0, 0);
    cf[f] = make_float4(coef[4 * (size_t)f], coef[4 * (size_t)f + 1], coef[4 * (size_t)f + 2], coef[4 * (size_t)f + 3]);
  }
  if (sparse_doubles(keys)) return fdtd_fail(c, FDTD_E_ARG, "fdtd_conformal_set: a face given twice");
  if (int r = correction_set_replace(c, corr_conformal)) return r;
  if (n == 0) return FDTD_OK;
  hipError_t e = to_device(&c->conf_face, face);
  if (e == hipSuccess) e = to_device(&c->conf_coef, cf);
  if (e == hipSuccess) e = hipMalloc((void**)&c->conf_iprev, (size_t)n * sizeof(float));
  if (e != hipSuccess) return correction_set_failed(c, corr_conformal, "fdtd_conformal_set", e);
  c->conf_n = n;
  const int r = conformal_prime(c, -1);
  if (r) conformal_free(c);
  return r;
}

int fdtd_conformal_get(fdtd_ctx* c, float* i_prev, int* nfaces_out) {
  if (!c) return FDTD_E_ARG;
  HIPCK(c, hipSetDevice(c->d.device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  if (nfaces_out) *nfaces_out = c->conf_n;
  if (i_prev && c->conf_n > 0) HIPCK(c, hipMemcpy(i_prev, c->conf_iprev, (size_t)c->conf_n * sizeof(float), hipMemcpyDeviceToHost));
  return FDTD_OK;
}

}  // extern "C"
