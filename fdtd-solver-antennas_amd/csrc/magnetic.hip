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
#include "fdtd_ctx.h"
#include "kernel_common.hpp"
#include "../../include/fdtd_hip_magnetic.h"

#include <vector>

namespace {

constexpr int MTAB = FDTD_MAGNETIC_MAX_CLASSES + 1;   // table entries: the class byte indexes it directly, entry 0 is never used
static_assert(MTAB == 256, "k_magnetic stages one table entry per thread of its 256-thread blocks");

struct MagComp {
  float* I;                // the component's current array (local plane 0)
  float* iprev; const uint8_t* cls;
  unsigned blk0;           // first block of this component in the launch
  unsigned nq;             // threads = groups of four x-faces: nz_b * ny_b * qx
  int off0;                // field offset of the box's first face: z0 * plane + y0 * P + x0w
  FastDiv fd_qx, fd_ny;    // groups per row, rows per plane
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
  const unsigned b = blockIdx.x;
  const int ci = b >= a.c[2].blk0 ? 2 : b >= a.c[1].blk0 ? 1 : 0;
  const MagComp& m = a.c[ci];
  const unsigned q = (b - m.blk0) * 256u + threadIdx.x;
  if (q >= m.nq) return;
  const size_t o = (size_t)q * 4u;                                                     // in the box arrays
  const unsigned c4 = *reinterpret_cast<const unsigned*>(m.cls + o);
  if (c4 == 0u) return;                                                                // (padding, or cells of another material inside the box)
  const unsigned row = fd_div(q, m.fd_qx);
  const unsigned ix = q - row * m.fd_qx.d;
  const unsigned kz = fd_div(row, m.fd_ny);
  const unsigned jy = row - kz * m.fd_ny.d;
  const long of = (long)m.off0 + (long)kz * a.plane + (long)jy * a.P + (long)ix * 4;   // in the field array
  float4 I4 = *reinterpret_cast<const float4*>(m.I + of);
  float4 p4 = *reinterpret_cast<const float4*>(m.iprev + o);
  magnetic_face(I4.x, p4.x, c4 & 0xffu, tab);
  magnetic_face(I4.y, p4.y, (c4 >> 8) & 0xffu, tab);
  magnetic_face(I4.z, p4.z, (c4 >> 16) & 0xffu, tab);
  magnetic_face(I4.w, p4.w, c4 >> 24, tab);
  *reinterpret_cast<float4*>(m.I + of) = I4;
  *reinterpret_cast<float4*>(m.iprev + o) = p4;
}

inline int floor4(int v) { return v & ~3; }
inline int ceil4(int v) { return (v + 3) & ~3; }

}  // namespace

void magnetic_free(fdtd_ctx* c) {
  for (auto& b : c->mag_box) {
    hipFree(b.iprev); hipFree(b.cls);
    b = fdtd_ctx::MagBox{};
  }
  hipFree(c->mag_tab);
  c->mag_tab = nullptr;
  c->mag_ncls = 0;
}

void launch_magnetic(fdtd_ctx* c, hipStream_t s) {
  if (c->mag_ncls <= 0) return;
  MagArgs a{};
  unsigned blocks = 0;
  for (int ci = 0; ci < 3; ++ci) {
    const fdtd_ctx::MagBox& b = c->mag_box[ci];
    MagComp& m = a.c[ci];
    m.blk0 = blocks;
    m.nq = (unsigned)(b.n / 4);
    m.fd_qx = make_fastdiv(1); m.fd_ny = make_fastdiv(1);
    if (b.n == 0) continue;
    m.I = c->p.I[ci]; m.iprev = b.iprev; m.cls = b.cls;
    m.off0 = b.lo[2] * c->plane + b.lo[1] * c->P + b.x0w;
    m.fd_qx = make_fastdiv((unsigned)(b.nxw / 4));
    m.fd_ny = make_fastdiv((unsigned)(b.hi[1] - b.lo[1]));
    blocks += (m.nq + 255u) / 256u;
  }
  if (blocks == 0) return;
  a.P = c->P; a.plane = c->plane; a.ntab = c->mag_ncls + 1; a.tab = c->mag_tab;
  hipLaunchKernelGGL(k_magnetic, dim3(blocks), dim3(256), 0, s, a);
}

// i_prev of component ci <- the I array over the widened box (fdtd_magnetic_set, fdtd_set_field(FDTD_KIND_I)): row by row, device to device
int magnetic_prime(fdtd_ctx* c, int ci) {
  const fdtd_ctx::MagBox& b = c->mag_box[ci];
  if (c->mag_ncls <= 0 || b.n == 0) return FDTD_OK;
  const int nyb = b.hi[1] - b.lo[1], nzb = b.hi[2] - b.lo[2];
  for (int z = 0; z < nzb; ++z)
    HIPCK(c, hipMemcpy2D(b.iprev + (size_t)z * nyb * b.nxw, (size_t)b.nxw * 4,
                         c->p.I[ci] + (size_t)(b.lo[2] + z) * c->plane + (size_t)b.lo[1] * c->P + b.x0w, (size_t)c->P * 4,
                         (size_t)b.nxw * 4, (size_t)nyb, hipMemcpyDeviceToDevice));
  return FDTD_OK;
}

extern "C" {

int fdtd_magnetic_set(fdtd_ctx* c, int ncls, const float* ta, const float* tb, const int32_t lo[3][3], const int32_t hi[3][3],
                      const uint8_t* const cls[3]) {
  if (!c) return FDTD_E_ARG;
  if (ncls < 0) return fdtd_fail(c, FDTD_E_ARG, "fdtd_magnetic_set: ncls %d", ncls);
  if (ncls > FDTD_MAGNETIC_MAX_CLASSES)
    return fdtd_fail(c, FDTD_E_UNSUPPORTED, "magnetic materials: %d distinct (a, b) classes, at most %d (one class byte per face)", ncls, FDTD_MAGNETIC_MAX_CLASSES);
  if (ncls > 0 && (!ta || !tb || !lo || !hi || !cls)) return fdtd_fail(c, FDTD_E_ARG, "fdtd_magnetic_set: bad argument");
  if (ncls > 0 && (c->d.world > 1 || c->p.p2p || c->link_lo || c->link_hi))
    return fdtd_fail(c, FDTD_E_UNSUPPORTED, "magnetic materials: single slab only (world = 1, no p2p transport, no linked contexts)");
  if (!c->have_op) return fdtd_fail(c, FDTD_E_STATE, "fdtd_magnetic_set: set the operator first");
  if (c->step != 0) return fdtd_fail(c, FDTD_E_STATE, "fdtd_magnetic_set: before the first timestep");
  const int nn[3] = {c->d.nx, c->d.ny, c->d.nz};
  size_t nbox[3] = {0, 0, 0};
  for (int ci = 0; ci < 3 && ncls > 0; ++ci) {
    bool empty = false;
    for (int a = 0; a < 3; ++a) empty = empty || hi[ci][a] <= lo[ci][a];
    if (empty) continue;
    for (int a = 0; a < 3; ++a)
      if (lo[ci][a] < 0 || hi[ci][a] > nn[a])
        return fdtd_fail(c, FDTD_E_ARG, "fdtd_magnetic_set: component %d: box [%d, %d) along axis %d leaves the grid", ci, lo[ci][a], hi[ci][a], a);
    if (!cls[ci]) return fdtd_fail(c, FDTD_E_ARG, "fdtd_magnetic_set: component %d: class bytes missing", ci);
    nbox[ci] = (size_t)(hi[ci][0] - lo[ci][0]) * (hi[ci][1] - lo[ci][1]) * (hi[ci][2] - lo[ci][2]);
    if (nbox[ci] * 4 > 0x7fffffffu) return fdtd_fail(c, FDTD_E_ARG, "fdtd_magnetic_set: component %d: box too large", ci);
    for (size_t e = 0; e < nbox[ci]; ++e)
      if (cls[ci][e] > ncls) return fdtd_fail(c, FDTD_E_ARG, "fdtd_magnetic_set: component %d: class %d out of range", ci, (int)cls[ci][e]);
  }
  HIPCK(c, hipSetDevice(c->d.device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  magnetic_free(c);
  if (ncls == 0 || nbox[0] + nbox[1] + nbox[2] == 0) return FDTD_OK;
  hipError_t e = hipSuccess;
  for (int ci = 0; ci < 3 && e == hipSuccess; ++ci) {
    if (nbox[ci] == 0) continue;
    fdtd_ctx::MagBox& b = c->mag_box[ci];
    for (int a = 0; a < 3; ++a) { b.lo[a] = lo[ci][a]; b.hi[a] = hi[ci][a]; }
    b.x0w = floor4(b.lo[0]);
    b.nxw = ceil4(b.hi[0]) - b.x0w;           // ceil4(hi) <= ceil4(nx) = P: the widened rows stay inside the field rows
    const int nyb = b.hi[1] - b.lo[1], nzb = b.hi[2] - b.lo[2], nxb = b.hi[0] - b.lo[0];
    b.n = (size_t)b.nxw * nyb * nzb;
    std::vector<uint8_t> cc(b.n, 0);
    for (size_t r = 0; r < (size_t)nyb * nzb; ++r)
      for (int x = 0; x < nxb; ++x) cc[r * b.nxw + (b.lo[0] - b.x0w) + x] = cls[ci][r * nxb + x];
    e = sparse_upload(&b.cls, cc);
    if (e == hipSuccess) e = hipMalloc((void**)&b.iprev, b.n * sizeof(float));
  }
  if (e == hipSuccess) {
    std::vector<float2> tab(MTAB, make_float2(1.0f, 1.0f));
    for (int q = 0; q < ncls; ++q) tab[q + 1] = make_float2(ta[q], tb[q]);
    e = sparse_upload(&c->mag_tab, tab);
  }
  if (e != hipSuccess) {
    magnetic_free(c);
    return fdtd_fail(c, e == hipErrorOutOfMemory ? FDTD_E_NOMEM : FDTD_E_DEVICE, "fdtd_magnetic_set: %s", hipGetErrorString(e));
  }
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
  if (c->mag_ncls == 0 || b.n == 0) return FDTD_OK;
  const int nyb = b.hi[1] - b.lo[1], nzb = b.hi[2] - b.lo[2], nxb = b.hi[0] - b.lo[0];
  const size_t rows = (size_t)nyb * nzb;
  if (i_prev) {
    std::vector<float> tmp(b.n);
    HIPCK(c, hipMemcpy(tmp.data(), b.iprev, b.n * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; ++r)
      for (int x = 0; x < nxb; ++x) i_prev[r * nxb + x] = tmp[r * b.nxw + (size_t)(b.lo[0] - b.x0w) + x];
  }
  if (iv0) {   // the faces' iv, as the update kernels expand it (raw or class form): the whole operator once, cropped to the box
    const size_t ncell = (size_t)c->d.nk * c->d.ny * c->d.nx;
    std::vector<float> op[4];
    for (auto& v : op) v.resize(3 * ncell);
    const int r = fdtd_get_operator(c, op[0].data(), op[1].data(), op[2].data(), op[3].data());
    if (r) return r;
    for (int z = 0; z < nzb; ++z)
      for (int y = 0; y < nyb; ++y)
        for (int x = 0; x < nxb; ++x)
          iv0[((size_t)z * nyb + y) * nxb + x] =
              op[3][(size_t)comp * ncell + ((size_t)(b.lo[2] + z) * c->d.ny + (b.lo[1] + y)) * c->d.nx + b.lo[0] + x];
  }
  return FDTD_OK;
}

}  // extern "C"
