// dense_box.hpp — what the dense-box corrections share (dispersion.hip, lorentz.hip: edges; magnetic.hip: faces).
//
// A volume effect is corrected densely: per field component one box of elements laid out like the field arrays, its x range widened
// to multiples of 4 (DenseBox, fdtd_ctx.h), one thread per four consecutive x-elements of a row, every array over the widened box
// moved as 16-byte vectors, consecutive lanes on consecutive memory, no index array.  Elements of the widening, and cells of another
// material inside the box, carry a neutral value (weight 0, class 0) and are left alone.  One launch covers the three components:
// blocks [blk0, blk0 + ceil(nq / 256)) belong to a component.  Here: the host side of the box (check, widen, scatter, crop, an operator
// array over it), the launch layout and the kernels' decode.
#pragma once
#include "corrections.hpp"
#include "kernel_common.hpp"

#include <vector>

// One component's share of a launch, as the kernel sees it
struct BoxLaunch {
  unsigned blk0;           // first block of this component in the launch
  unsigned nq;             // threads = groups of four x-elements: nz_b * ny_b * qx
  unsigned n;              // elements of the widened box = 4 * nq (stride of the state planes)
  int off0;                // field offset of the box's first element: z0 * plane + y0 * P + x0w
  FastDiv fd_qx, fd_ny;    // groups per row, rows per plane
};

namespace {

// block -> component (its BoxLaunch is comp[ci].l) and group q of four elements at offset 4 q of the box arrays; the caller returns when
// q >= nq ...
template <class Comp>
__device__ __forceinline__ const Comp& box_group(const Comp (&comp)[3], unsigned& q) {
  const unsigned b = blockIdx.x;
  const int ci = b >= comp[2].l.blk0 ? 2 : b >= comp[1].l.blk0 ? 1 : 0;
  const Comp& d = comp[ci];
  q = (b - d.l.blk0) * 256u + threadIdx.x;
  return d;
}
// ... and group -> offset of its first element in the field array (k_magnetic looks at its class bytes in between)
__device__ __forceinline__ long box_field_offset(const BoxLaunch& l, const unsigned q, const int P, const int plane) {
  const unsigned row = fd_div(q, l.fd_qx);
  const unsigned ix = q - row * l.fd_qx.d;
  const unsigned kz = fd_div(row, l.fd_ny);
  const unsigned jy = row - kz * l.fd_ny.d;
  return (long)l.off0 + (long)kz * plane + (long)jy * P + (long)ix * 4;
}

inline int floor4(int v) { return v & ~3; }
inline int ceil4(int v) { return (v + 3) & ~3; }

// Fills comp[ci].l from box[ci].g and returns the blocks of the launch; a component without elements takes no block
template <class Box, class Comp>
unsigned box_layout(const fdtd_ctx* c, const Box (&box)[3], Comp (&comp)[3]) {
  unsigned blocks = 0;
  for (int ci = 0; ci < 3; ++ci) {
    const DenseBox& g = box[ci].g;
    BoxLaunch& l = comp[ci].l;
    l.blk0 = blocks;
    l.nq = (unsigned)(g.n / 4);
    l.n = (unsigned)g.n;
    l.fd_qx = make_fastdiv(1); l.fd_ny = make_fastdiv(1);
    if (g.n == 0) continue;
    l.off0 = g.lo[2] * c->plane + g.lo[1] * c->P + g.x0w;
    l.fd_qx = make_fastdiv((unsigned)(g.nxw / 4));
    l.fd_ny = make_fastdiv((unsigned)(g.hi[1] - g.lo[1]));
    blocks += (l.nq + 255u) / 256u;
  }
  return blocks;
}

// The caller's box of component ci: *nbox = 0 when it is empty, else it lies inside the grid (`faces`: up to n along the component's own
// axis, edges: to n - 1; `noun`: what it leaves otherwise), its arrays are there (`have`, else `missing`) and it is not too large
int box_check(fdtd_ctx* c, const char* who, int ci, const int32_t lo[3], const int32_t hi[3], bool faces, const char* noun, bool have,
              const char* missing, size_t* nbox) {
  const int nn[3] = {c->d.nx, c->d.ny, c->d.nz};
  *nbox = 0;
  for (int a = 0; a < 3; ++a)
    if (hi[a] <= lo[a]) return FDTD_OK;
  for (int a = 0; a < 3; ++a)
    if (lo[a] < 0 || hi[a] > (a == ci && !faces ? nn[a] - 1 : nn[a]))
      return fdtd_fail(c, FDTD_E_ARG, "%s: component %d: box [%d, %d) along axis %d leaves the %s", who, ci, lo[a], hi[a], a, noun);
  if (!have) return fdtd_fail(c, FDTD_E_ARG, "%s: component %d: %s missing", who, ci, missing);
  *nbox = (size_t)(hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]);
  if (*nbox * 4 > 0x7fffffffu) return fdtd_fail(c, FDTD_E_ARG, "%s: component %d: box too large", who, ci);
  return FDTD_OK;
}

DenseBox box_widen(const int32_t lo[3], const int32_t hi[3]) {
  DenseBox g;
  for (int a = 0; a < 3; ++a) { g.lo[a] = lo[a]; g.hi[a] = hi[a]; }
  g.x0w = floor4(g.lo[0]);
  g.nxw = ceil4(g.hi[0]) - g.x0w;           // ceil4(hi) <= ceil4(nx) = P: the widened rows stay inside the field rows
  g.n = (size_t)g.nxw * (g.hi[1] - g.lo[1]) * (g.hi[2] - g.lo[2]);
  return g;
}

// the caller's [z][y][x] over the box -> the widened box, zeros in the widening
template <class T>
std::vector<T> scatter(const DenseBox& g, const T* src) {
  const int nxb = g.hi[0] - g.lo[0];
  const size_t rows = (size_t)(g.hi[1] - g.lo[1]) * (g.hi[2] - g.lo[2]);
  std::vector<T> out(g.n, T(0));
  for (size_t r = 0; r < rows; ++r)
    for (int x = 0; x < nxb; ++x) out[r * g.nxw + (g.lo[0] - g.x0w) + x] = src[r * nxb + x];
  return out;
}

// a device array over the widened box -> the caller's [z][y][x] over the box
hipError_t crop(const DenseBox& g, const float* dev, float* out) {
  std::vector<float> tmp(g.n);
  const hipError_t e = hipMemcpy(tmp.data(), dev, g.n * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  const int nxb = g.hi[0] - g.lo[0];
  const size_t rows = (size_t)(g.hi[1] - g.lo[1]) * (g.hi[2] - g.lo[2]);
  for (size_t r = 0; r < rows; ++r)
    for (int x = 0; x < nxb; ++x) out[r * nxb + x] = tmp[r * g.nxw + (size_t)(g.lo[0] - g.x0w) + x];
  return hipSuccess;
}

// Array `which` of the operator (1: vi, 3: iv) as the update kernels expand it (raw or class form), [3][nk][ny][nx]: the whole operator once ...
int operator_array(fdtd_ctx* c, int which, std::vector<float>* out) {
  const size_t ncell = (size_t)c->d.nk * c->d.ny * c->d.nx;
  std::vector<float> op[4];
  for (auto& v : op) v.resize(3 * ncell);
  const int r = fdtd_get_operator(c, op[0].data(), op[1].data(), op[2].data(), op[3].data());
  if (r == FDTD_OK) out->swap(op[which]);
  return r;
}
// ... cropped to component ci's box, [z][y][x]
void operator_over_box(const fdtd_ctx* c, const std::vector<float>& whole, int ci, const DenseBox& g, float* out) {
  const size_t ncell = (size_t)c->d.nk * c->d.ny * c->d.nx;
  const int nxb = g.hi[0] - g.lo[0], nyb = g.hi[1] - g.lo[1], nzb = g.hi[2] - g.lo[2];
  for (int z = 0; z < nzb; ++z)
    for (int y = 0; y < nyb; ++y)
      for (int x = 0; x < nxb; ++x)
        out[((size_t)z * nyb + y) * nxb + x] = whole[(size_t)ci * ncell + ((size_t)(g.lo[2] + z) * c->d.ny + (g.lo[1] + y)) * c->d.nx + g.lo[0] + x];
}

}  // namespace

// dispersion.hip: the host side of the Debye media, which the Lorentz media share.  `planes`: state planes per pole (1, 2); `tab`: the
// packed table as the kernel reads it; `row`: the caller's own.  The exported setters check their own limits and pack their own tables.
void media_free(MediaBoxes* m);
int media_set(fdtd_ctx* c, MediaBoxes* m, const CorrectionRow& row, const char* who, int planes, int nmedia, int K, const std::vector<float>& tab,
              const int32_t lo[3][3], const int32_t hi[3][3], const float* const w[3], const uint8_t* const med[3]);
int media_get(fdtd_ctx* c, const MediaBoxes* m, const char* who, int planes, int comp, float* v_prev, float* u, float* vi);
