// magnetic.hip — magnetic materials: mu_r >= 1 and magnetic loss on the face currents (include/fdtd_hip_magnetic.h).
//
// The operator and the H kernels stay what they are (ii = 1, iv0); what a magnetic face needs, I <- a I + b iv0 curl, is restored by
// a correction after the H update of every timestep: the H update has left I = i_prev + iv0 curl, so a (i_prev) + b (I - i_prev) is
// the wanted value.  Like the Debye media it is a VOLUME effect, so it is dense: per field component one box of faces laid out like
// the field arrays, one thread per four consecutive x-faces of a row, I and i_prev moved as 16-byte vectors, the four class bytes as
// one dword, consecutive lanes on consecutive memory, no index array.  Per face the kernel moves 8 (I) + 8 (i_prev) + 1 (class)
// bytes and does 4 flops: it is a streaming kernel.  The (a, b) table of at most 256 classes is staged in LDS (2 KiB).  Every
// statement is one fp32 operation in the order the header spells (-ffp-contract=off), so a host restatement on top of the oracle's
// half-steps reproduces it bit for bit.
#include "dense_box.hpp"
#include "../../include/fdtd_hip_magnetic.h"

#include <vector>

namespace {

constexpr int MTAB = FDTD_MAGNETIC_MAX_CLASSES + 1;   // table entries: the class byte indexes it directly, entry 0 is never used
static_assert(MTAB == 256, "k_magnetic stages one table entry per thread of its 256-thread blocks");

struct MagComp {
  float* I;                // the component's current array (local plane 0)
  float* iprev; const uint8_t* cls;
  BoxLaunch l;
};
struct MagArgs { MagComp c[3]; int P, plane, ntab; const float2* tab; };

// One lane of the correction (the header's statement list).  Class 0: nothing changes.
__device__ __forceinline__ void magnetic_face(float& I, float& ip, const unsigned cl, const float2* tab) {
  const float2 ab = tab[cl];
  const float d = I - ip;
  const float p = ab.x * ip;
  const float q = ab.y * d;
  const float r = p + q;
  const bool on = cl != 0u;
  I = on ? r : I;
  ip = on ? r : ip;
}

__global__ __launch_bounds__(256) void k_magnetic(const MagArgs a) {
  __shared__ float2 tab[MTAB];
  tab[threadIdx.x] = (int)threadIdx.x < a.ntab ? a.tab[threadIdx.x] : make_float2(1.0f, 1.0f);
  __syncthreads();
  unsigned q;
  const MagComp& m = box_group(a.c, q);
  if (q >= m.l.nq) return;
  const size_t o = (size_t)q * 4u;                                                     // in the box arrays
  const unsigned c4 = *reinterpret_cast<const unsigned*>(m.cls + o);
  if (c4 == 0u) return;                                                                // (padding, or cells of another material inside the box)
  const long of = box_field_offset(m.l, q, a.P, a.plane);                              // in the field array
  float4 I4 = *reinterpret_cast<const float4*>(m.I + of);
  float4 p4 = *reinterpret_cast<const float4*>(m.iprev + o);
  magnetic_face(I4.x, p4.x, c4 & 0xffu, tab);
  magnetic_face(I4.y, p4.y, (c4 >> 8) & 0xffu, tab);
  magnetic_face(I4.z, p4.z, (c4 >> 16) & 0xffu, tab);
  magnetic_face(I4.w, p4.w, c4 >> 24, tab);
  *reinterpret_cast<float4*>(m.I + of) = I4;
  *reinterpret_cast<float4*>(m.iprev + o) = p4;
}

void magnetic_free(fdtd_ctx* c) {
  for (auto& b : c->mag_box) {
    hipFree(b.iprev); hipFree(b.cls);
    b = fdtd_ctx::MagBox{};
  }
  hipFree(c->mag_tab);
  c->mag_tab = nullptr;
  c->mag_ncls = 0;
}

void launch_magnetic(fdtd_ctx* c, long long, hipStream_t s) {
  if (c->mag_ncls <= 0) return;
  MagArgs a{};
  const unsigned blocks = box_layout(c, c->mag_box, a.c);
  if (blocks == 0) return;
  for (int ci = 0; ci < 3; ++ci) {
    const fdtd_ctx::MagBox& b = c->mag_box[ci];
    if (b.g.n == 0) continue;
    MagComp& m = a.c[ci];
    m.I = c->p.I[ci]; m.iprev = b.iprev; m.cls = b.cls;
  }
  a.P = c->P; a.plane = c->plane; a.ntab = c->mag_ncls + 1; a.tab = c->mag_tab;
  hipLaunchKernelGGL(k_magnetic, dim3(blocks), dim3(256), 0, s, a);
}

// i_prev of component ci <- the I array over the widened box (fdtd_magnetic_set, fdtd_set_field(FDTD_KIND_I)): row by row, device to device
int magnetic_prime(fdtd_ctx* c, int ci) {
  const fdtd_ctx::MagBox& b = c->mag_box[ci];
  const DenseBox& g = b.g;
  if (c->mag_ncls <= 0 || g.n == 0) return FDTD_OK;
  const int nyb = g.hi[1] - g.lo[1], nzb = g.hi[2] - g.lo[2];
  for (int z = 0; z < nzb; ++z)
    HIPCK(c, hipMemcpy2D(b.iprev + (size_t)z * nyb * g.nxw, (size_t)g.nxw * 4,
                         c->p.I[ci] + (size_t)(g.lo[2] + z) * c->plane + (size_t)g.lo[1] * c->P + g.x0w, (size_t)c->P * 4,
                         (size_t)g.nxw * 4, (size_t)nyb, hipMemcpyDeviceToDevice));
  return FDTD_OK;
}

}  // namespace

#ifndef __HIP_DEVICE_COMPILE__   // (host data: corrections.hpp)
const CorrectionRow corr_magnetic = {
    "magnetic materials", /*no_links*/ true, /*volume*/ false,
    [](const fdtd_ctx* c) { return c->mag_ncls > 0; },
    nullptr, launch_magnetic, magnetic_free, nullptr, magnetic_prime};
#endif

extern "C" {

int fdtd_magnetic_set(fdtd_ctx* c, int ncls, const float* ta, const float* tb, const int32_t lo[3][3], const int32_t hi[3][3],
                      const uint8_t* const cls[3]) {
  if (!c) return FDTD_E_ARG;
  if (ncls < 0) return fdtd_fail(c, FDTD_E_ARG, "fdtd_magnetic_set: ncls %d", ncls);
  if (ncls > FDTD_MAGNETIC_MAX_CLASSES)
    return fdtd_fail(c, FDTD_E_UNSUPPORTED, "magnetic materials: %d distinct (a, b) classes, at most %d (one class byte per face)", ncls, FDTD_MAGNETIC_MAX_CLASSES);
  if (ncls > 0 && (!ta || !tb || !lo || !hi || !cls)) return fdtd_fail(c, FDTD_E_ARG, "fdtd_magnetic_set: bad argument");
  if (int r = correction_set_begin(c, corr_magnetic, "fdtd_magnetic_set", ncls > 0)) return r;
  size_t nbox[3] = {0, 0, 0};
  for (int ci = 0; ci < 3 && ncls > 0; ++ci) {
    if (int r = box_check(c, "fdtd_magnetic_set", ci, lo[ci], hi[ci], true, "grid", cls[ci] != nullptr, "class bytes", &nbox[ci])) return r;
    for (size_t e = 0; e < nbox[ci]; ++e)
      if (cls[ci][e] > ncls) return fdtd_fail(c, FDTD_E_ARG, "fdtd_magnetic_set: component %d: class %d out of range", ci, (int)cls[ci][e]);
  }
  if (int r = correction_set_replace(c, corr_magnetic)) return r;
  if (ncls == 0 || nbox[0] + nbox[1] + nbox[2] == 0) return FDTD_OK;
  hipError_t e = hipSuccess;
  for (int ci = 0; ci < 3 && e == hipSuccess; ++ci) {
    if (nbox[ci] == 0) continue;
    fdtd_ctx::MagBox& b = c->mag_box[ci];
    b.g = box_widen(lo[ci], hi[ci]);
    e = to_device(&b.cls, scatter(b.g, cls[ci]));
    if (e == hipSuccess) e = hipMalloc((void**)&b.iprev, b.g.n * sizeof(float));
  }
  if (e == hipSuccess) {
    std::vector<float2> tab(MTAB, make_float2(1.0f, 1.0f));
    for (int q = 0; q < ncls; ++q) tab[q + 1] = make_float2(ta[q], tb[q]);
    e = to_device(&c->mag_tab, tab);
  }
  if (e != hipSuccess) return correction_set_failed(c, corr_magnetic, "fdtd_magnetic_set", e);
  c->mag_ncls = ncls;
  for (int ci = 0; ci < 3; ++ci) {
    const int r = magnetic_prime(c, ci);
    if (r) { magnetic_free(c); return r; }
  }
  return FDTD_OK;
}

int fdtd_magnetic_get(fdtd_ctx* c, int comp, float* i_prev, float* iv0) {
  if (!c) return FDTD_E_ARG;
  if (comp < 0 || comp > 2) return fdtd_fail(c, FDTD_E_ARG, "fdtd_magnetic_get: component %d", comp);
  HIPCK(c, hipSetDevice(c->d.device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  const fdtd_ctx::MagBox& b = c->mag_box[comp];
  if (c->mag_ncls == 0 || b.g.n == 0) return FDTD_OK;
  if (i_prev) HIPCK(c, crop(b.g, b.iprev, i_prev));
  if (iv0) {
    std::vector<float> iv;
    if (int r = operator_array(c, 3, &iv)) return r;
    operator_over_box(c, iv, comp, b.g, iv0);
  }
  return FDTD_OK;
}

}  // extern "C"
