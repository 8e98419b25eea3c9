// voxel.hip — rasterise the primitive table of include/fdtd_hip_voxel.h onto the Yee grid (what scene.voxelize did in numpy over
// whole-grid temporaries).  One kernel, templated on the pass: the cell pass tests cell centres against the material records and
// keeps the winner; the edge pass tests every node and its +x, +y, +z neighbours against the metal records and keeps the winner
// per component.  Triangle meshes (POLYHEDRON records) run in a second launch of the same kernel (POLY = true: the same tile, point map
// and single writer, starting from the owners the first launch stored), so the registers of the first stay sized by the analytic
// types; a table without a mesh launches what it always did.  float64 throughout, in the operation order the header spells (primitives._inside is the same text in numpy;
// -ffp-contract=off keeps the compiler from fusing), so the owners are those of primitives.rasterise_spec bit for bit.
// Records that delimit a voxel map (fdtd_voxelize_maps) take a third launch, k_voxel_map below, which merges them into those owners.
//
// A block of 256 threads owns a tile of one z-plane: VX_TY rows of VX_TX threads, four consecutive x points per thread.  The table
// is staged through LDS in chunks of VX_CHUNK records; a record whose index box misses the block's tile is skipped before any
// arithmetic (block-uniform: the record's integers go through readfirstlane, so the skip is a scalar branch) — N primitives x M
// points becomes about M.  Every output word has exactly one writer and is always written (-1: no owner): no atomics, no memset.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "fdtd_ctx.h"
#include "../../include/fdtd_hip_voxel.h"
#include "../../include/fdtd_hip_conformal.h"

static_assert(sizeof(fdtd_voxel_prim) == 248, "fdtd_voxel_prim is 248 bytes (primitives.RECORD)");

namespace {
constexpr int VX_BLOCK = 256, VX_TX = 32, VX_TY = 8, VX_PTS = 4;
constexpr int VX_CHUNK = 48;                                  // records per LDS chunk: 48 * 248 B = 11.6 KiB
constexpr int VX_WORDS = (int)(sizeof(fdtd_voxel_prim) / 8);  // 31
constexpr int VX_TRI_CHUNK = VX_BLOCK;                        // triangles per chunk, one per thread: 256 * 72 B = 18 KiB of LDS
enum { PASS_CELL = 0, PASS_EDGE = 1 };

struct VoxArgs {
  int nx, ny, nz;             // node counts
  const double* lines;        // x lines, y lines, z lines
  int nprim;
  const fdtd_voxel_prim* table;
  const double* verts;
  double tol;
  int32_t* out;               // cell pass: [nz-1][ny-1][nx-1]; edge pass: [3][nz][ny][nx]
};

// the points of one thread: cell pass 4 (x + q); edge pass 13: q 0..4 at x + q, 5..8 at (x + q - 5, y + 1), 9..12 at (x + q - 9, z + 1)
template <int PASS> struct PtMap {
  static constexpr int N = PASS == PASS_CELL ? 4 : 13;
  static constexpr __host__ __device__ int xi(int q) { return q < 5 ? q : (q < 9 ? q - 5 : q - 9); }
  static constexpr __host__ __device__ int yi(int q) { return (q >= 5 && q < 9) ? 1 : 0; }
  static constexpr __host__ __device__ int zi(int q) { return q >= 9 ? 1 : 0; }
};

// point-to-segment distance^2 <= lim2 (w = p - a, g = p - b, d = b - a), division-free
__device__ __forceinline__ bool seg_near(double wx, double wy, double wz, double gx, double gy, double gz, double dx, double dy,
                                         double dz, double lim2) {
  const double L = (dx * dx + dy * dy) + dz * dz;
  const double s = (wx * dx + wy * dy) + wz * dz;
  const double ww = (wx * wx + wy * wy) + wz * wz;
  const double gg = (gx * gx + gy * gy) + gz * gz;
  return s <= 0.0 ? ww <= lim2 : (s >= L ? gg <= lim2 : ww * L - s * s <= lim2 * L);
}

// ---- POLYHEDRON (include/fdtd_hip_voxel.h): a closed triangle mesh, parity of the crossings of the ray towards +x ---------------
// ((b - a) x (p - a)) . n >= 0: p is on the inner side of the triangle's edge a -> b
__device__ __forceinline__ bool tri_side(double ax, double ay, double az, double bx, double by, double bz, double px, double py,
                                         double pz, double nx, double ny, double nz) {
  const double dx = bx - ax, dy = by - ay, dz = bz - az;
  const double vx = px - ax, vy = py - ay, vz = pz - az;
  const double cx = dy * vz - dz * vy, cy = dz * vx - dx * vz, cz = dx * vy - dy * vx;
  return (cx * nx + cy * ny) + cz * nz >= 0.0;
}
// one crossing of the projected edge P -> Q, its end points taken in canonical order (the smaller z first, then the smaller y)
__device__ __forceinline__ bool tri_cross(double Py, double Pz, double Qy, double Qz, double y, double z) {
  const bool sw = Qz < Pz || (Qz == Pz && Qy < Py);
  const double ay = sw ? Qy : Py, az = sw ? Qz : Pz, by = sw ? Py : Qy, bz = sw ? Pz : Qz;
  const double du = by - ay, dv = bz - az, wu = y - ay, wv = z - az;
  return ((az > z) != (bz > z)) && (wu * dv < wv * du);
}
// Records are in drawing order, so within one launch >= lets the later one win a tie; the polyhedron launch meets owners of either side.
template <bool POLY> __device__ __forceinline__ bool vx_wins(int prio, int idx, int best, int own) {
  return POLY ? (prio > best || (prio == best && idx > own)) : prio >= best;
}
// The points of a caller that share (y, z) with an earlier one (PtMap: the cell pass's four, the edge pass's 5 + 4 + 4) take its
// gate and its projected hit when the record has no transform: the earlier point's index.
template <int N> constexpr __host__ __device__ int vx_yz_rep(int q) { return N == 4 ? 0 : (N == 13 ? (q < 5 ? 0 : (q < 9 ? 5 : 9)) : q); }

// the gate of a triangle T[9]: its (y, z) bounding box grown by g
__device__ __forceinline__ void tri_gate(const double* T, const double g, double& y0, double& y1, double& z0, double& z1) {
  const double ay = T[1], az = T[2], by = T[4], bz = T[5], cy = T[7], cz = T[8];
  const double ymn = ay < by ? ay : by, ymx = ay > by ? ay : by, zmn = az < bz ? az : bz, zmx = az > bz ? az : bz;
  y0 = (ymn < cy ? ymn : cy) - g; y1 = (ymx > cy ? ymx : cy) + g;
  z0 = (zmn < cz ? zmn : cz) - g; z1 = (zmx > cz ? zmx : cz) + g;
}

// ntri triangles at V (global memory or LDS; every lane reads the same one) on the N local points: par ^= crossings, near |= within tol
template <int N>
__device__ __forceinline__ void vx_tris(const double* V, const int ntri, const bool has_matrix, const double tol, const double (&x)[N],
                                        const double (&y)[N], const double (&z)[N], const unsigned gate, unsigned& par, unsigned& near) {
  const double tol2 = tol * tol, g = 2.0 * tol;
  for (int tr = 0; tr < ntri; ++tr) {
    const double* T = V + 9 * (size_t)tr;
    const double ax = T[0], ay = T[1], az = T[2], bx = T[3], by = T[4], bz = T[5], cx = T[6], cy = T[7], cz = T[8];
    double y0, y1, z0, z1;
    tri_gate(T, g, y0, y1, z0, z1);
    unsigned inyz = 0u;
#pragma unroll
    for (int q = 0; q < N; ++q) {
      const int rq = vx_yz_rep<N>(q);
      bool b;
      if (rq != q && !has_matrix) b = (inyz >> rq) & 1u;
      else b = ((y[q] >= y0) && (y[q] <= y1)) && ((z[q] >= z0) && (z[q] <= z1));
      inyz |= (b ? 1u : 0u) << q;
    }
    if ((inyz & gate) == 0u) continue;                           // the triangle's (y, z) box misses every point of this lane
    const double e1x = bx - ax, e1y = by - ay, e1z = bz - az, e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double nn = (nx * nx + ny * ny) + nz * nz;
    if (nx != 0.0) {
      unsigned proj = 0u;
#pragma unroll
      for (int q = 0; q < N; ++q) {
        const int rq = vx_yz_rep<N>(q);
        bool b;
        if (rq != q && !has_matrix) b = (proj >> rq) & 1u;
        else b = (tri_cross(ay, az, by, bz, y[q], z[q]) != tri_cross(by, bz, cy, cz, y[q], z[q])) != tri_cross(cy, cz, ay, az, y[q], z[q]);
        proj |= (b ? 1u : 0u) << q;
      }
      proj &= inyz;
#pragma unroll
      for (int q = 0; q < N; ++q) {
        const double wx = x[q] - ax, wy = y[q] - ay, wz = z[q] - az;
        const double s = (nx * wx + ny * wy) + nz * wz;
        const bool c = ((proj >> q) & 1u) && (nx > 0.0 ? s < 0.0 : s > 0.0);
        par ^= (c ? 1u : 0u) << q;
      }
    }
    const double xmn = ax < bx ? ax : bx, xmx = ax > bx ? ax : bx;
    const double x0 = (xmn < cx ? xmn : cx) - g, x1 = (xmx > cx ? xmx : cx) + g;
#pragma unroll
    for (int q = 0; q < N; ++q) {
      if (!((inyz & gate & ~near) >> q & 1u) || !((x[q] >= x0) && (x[q] <= x1))) continue;   // near is an OR: a held bit needs no test
      const double wx = x[q] - ax, wy = y[q] - ay, wz = z[q] - az;
      const double s = (nx * wx + ny * wy) + nz * wz;
      const bool c0 = tri_side(ax, ay, az, bx, by, bz, x[q], y[q], z[q], nx, ny, nz);
      const bool c1 = tri_side(bx, by, bz, cx, cy, cz, x[q], y[q], z[q], nx, ny, nz);
      const bool c2 = tri_side(cx, cy, cz, ax, ay, az, x[q], y[q], z[q], nx, ny, nz);
      bool nr;
      if (c0 && c1 && c2) {
        nr = s * s <= tol2 * nn;
      } else {
        const double ux = x[q] - bx, uy = y[q] - by, uz = z[q] - bz, tx = x[q] - cx, ty = y[q] - cy, tz = z[q] - cz;
        nr = seg_near(wx, wy, wz, ux, uy, uz, bx - ax, by - ay, bz - az, tol2) ||
             seg_near(ux, uy, uz, tx, ty, tz, cx - bx, cy - by, cz - bz, tol2) ||
             seg_near(tx, ty, tz, wx, wy, wz, ax - cx, ay - cy, az - cz, tol2);
      }
      near |= (nr ? 1u : 0u) << q;
    }
  }
}

template <int N>
__device__ __forceinline__ unsigned vx_poly(const bool metal, const int vert0, const int nvert, const bool has_matrix,
                                            const double* __restrict__ verts, const double tol, const double (&x)[N],
                                            const double (&y)[N], const double (&z)[N], const unsigned gate) {
  unsigned par = 0u, near = 0u;
  vx_tris<N>(verts + vert0, nvert / 3, has_matrix, tol, x, y, z, gate, par, near);
  return metal ? (par | near) : (par & ~near);
}

// Bit q of the result: point q is inside record r (in LDS) under its role's rule.  `gate` masks the points outside the index box.
// POLY = false leaves the POLYHEDRON case out (k_voxel<pass, false>; k_voxel<pass, true> takes those records, through vx_tris).
template <int N, bool POLY = true>
__device__ __forceinline__ unsigned vx_test(const fdtd_voxel_prim* r, const int type, const bool metal, const int norm_dir,
                                            const int vert0, const int nvert, const bool has_matrix,
                                            const double* __restrict__ verts, const double tol, const double (&wx)[N],
                                            const double (&wy)[N], const double (&wz)[N], const unsigned gate) {
  const double t = metal ? tol : -tol;
  double x[N], y[N], z[N];
  if (has_matrix) {
    const double m0 = r->m[0], m1 = r->m[1], m2 = r->m[2], m3 = r->m[3], m4 = r->m[4], m5 = r->m[5], m6 = r->m[6], m7 = r->m[7],
                 m8 = r->m[8], m9 = r->m[9], m10 = r->m[10], m11 = r->m[11];
#pragma unroll
    for (int q = 0; q < N; ++q) {
      x[q] = ((m0 * wx[q] + m1 * wy[q]) + m2 * wz[q]) + m3;
      y[q] = ((m4 * wx[q] + m5 * wy[q]) + m6 * wz[q]) + m7;
      z[q] = ((m8 * wx[q] + m9 * wy[q]) + m10 * wz[q]) + m11;
    }
  } else {
#pragma unroll
    for (int q = 0; q < N; ++q) { x[q] = wx[q]; y[q] = wy[q]; z[q] = wz[q]; }
  }
  const double p0 = r->par[0], p1 = r->par[1], p2 = r->par[2], p3 = r->par[3], p4 = r->par[4], p5 = r->par[5], p6 = r->par[6],
               p7 = r->par[7];
  if constexpr (POLY) {
    if (type == FDTD_VOXEL_POLYHEDRON) return vx_poly<N>(metal, vert0, nvert, has_matrix, verts, tol, x, y, z, gate) & gate;
  }
  unsigned in = 0u;
  switch (type) {
    case FDTD_VOXEL_BOX: {
#pragma unroll
      for (int q = 0; q < N; ++q) {
        const bool b = ((x[q] >= p0 - t) && (x[q] <= p3 + t)) && ((y[q] >= p1 - t) && (y[q] <= p4 + t)) &&
                       ((z[q] >= p2 - t) && (z[q] <= p5 + t));
        in |= (b ? 1u : 0u) << q;
      }
    } break;
    case FDTD_VOXEL_SPHERE:
    case FDTD_VOXEL_SPHERICAL_SHELL: {
      const bool shell = type == FDTD_VOXEL_SPHERICAL_SHELL;
      const double ro = shell ? (p3 + 0.5 * p4) + t : p3 + t;
      const double ri = shell ? (p3 - 0.5 * p4) - t : 0.0;
      const double ro2 = ro * ro, ri2 = ri * ri;
      if (ro >= 0.0) {
#pragma unroll
        for (int q = 0; q < N; ++q) {
          const double dx = x[q] - p0, dy = y[q] - p1, dz = z[q] - p2;
          const double d2 = (dx * dx + dy * dy) + dz * dz;
          const bool b = (d2 <= ro2) && (ri <= 0.0 || d2 >= ri2);
          in |= (b ? 1u : 0u) << q;
        }
      }
    } break;
    case FDTD_VOXEL_CYLINDER:
    case FDTD_VOXEL_CYLINDRICAL_SHELL: {
      const bool shell = type == FDTD_VOXEL_CYLINDRICAL_SHELL;
      const double dx = p3 - p0, dy = p4 - p1, dz = p5 - p2;
      const double L = (dx * dx + dy * dy) + dz * dz;
      const double tt = (tol * tol) * L;
      const double ro = shell ? (p6 + 0.5 * p7) + t : p6 + t;
      const double ri = shell ? (p6 - 0.5 * p7) - t : 0.0;
      const double ro2L = (ro * ro) * L, ri2L = (ri * ri) * L;
      if (ro >= 0.0) {
#pragma unroll
        for (int q = 0; q < N; ++q) {
          const double ax = x[q] - p0, ay = y[q] - p1, az = z[q] - p2;
          const double s = (ax * dx + ay * dy) + az * dz;
          const double ww = (ax * ax + ay * ay) + az * az;
          const double qq = ww * L - s * s;
          const double e = s - L;
          const bool axial = metal ? ((s >= 0.0 || s * s <= tt) && (e <= 0.0 || e * e <= tt))
                                   : ((s >= 0.0 && s * s >= tt) && (e <= 0.0 && e * e >= tt));
          const bool b = axial && (qq <= ro2L) && (ri <= 0.0 || qq >= ri2L);
          in |= (b ? 1u : 0u) << q;
        }
      }
    } break;
    case FDTD_VOXEL_DISC: {
      if (metal) {
        const double re = p6 + t;
        const double re2 = re * re;
#pragma unroll
        for (int q = 0; q < N; ++q) {
          const double dx = x[q] - p0, dy = y[q] - p1, dz = z[q] - p2;
          const bool b = ((dz <= tol) && (dz >= -tol)) && (dx * dx + dy * dy <= re2);
          in |= (b ? 1u : 0u) << q;
        }
      }
    } break;
    case FDTD_VOXEL_POLYGON:
    case FDTD_VOXEL_LINPOLY: {
      const bool flat = type == FDTD_VOXEL_POLYGON;
      if (flat && !metal) break;
      const double tol2 = tol * tol;
      unsigned nrm = 0u, par = 0u, near = 0u;
      double pu[N], pv[N];
#pragma unroll
      for (int q = 0; q < N; ++q) {
        const double pn = norm_dir == 0 ? x[q] : (norm_dir == 1 ? y[q] : z[q]);
        pu[q] = norm_dir == 0 ? y[q] : (norm_dir == 1 ? z[q] : x[q]);
        pv[q] = norm_dir == 0 ? z[q] : (norm_dir == 1 ? x[q] : y[q]);
        const double dn = pn - p0;
        const bool b = flat ? ((dn <= tol) && (dn >= -tol)) : ((pn >= p0 - t) && (pn <= p1 + t));
        nrm |= (b ? 1u : 0u) << q;
      }
      const double* V = verts + vert0;
      for (int e = 0; e < nvert; ++e) {
        const int f = e + 1 == nvert ? 0 : e + 1;
        const double au = V[2 * e], av = V[2 * e + 1], bu = V[2 * f], bv = V[2 * f + 1];
        const double du = bu - au, dv = bv - av;
        const double L = du * du + dv * dv;
#pragma unroll
        for (int q = 0; q < N; ++q) {
          const double wu = pu[q] - au, wv = pv[q] - av;
          const double lhs = wu * dv, rhs = wv * du;
          const bool straddle = (av > pv[q]) != (bv > pv[q]);
          const bool c = straddle && (dv > 0.0 ? lhs < rhs : lhs > rhs);
          par ^= (c ? 1u : 0u) << q;
          const double eu = pu[q] - bu, ev = pv[q] - bv;
          const double s = wu * du + wv * dv;
          const double ww = wu * wu + wv * wv;
          const double ee = eu * eu + ev * ev;
          const bool nr = s <= 0.0 ? ww <= tol2 : (s >= L ? ee <= tol2 : ww * L - s * s <= tol2 * L);
          near |= (nr ? 1u : 0u) << q;
        }
      }
      in = nrm & (metal ? (par | near) : (par & ~near));
    } break;
    case FDTD_VOXEL_WIRE: {
      const double re = p0 + t;
      if (!metal || re < 0.0) break;
      const double re2 = re * re;
      const double* V = verts + vert0;
      const int nseg = nvert > 1 ? nvert - 1 : 1;
      for (int e = 0; e < nseg; ++e) {
        const int f = e + 1 < nvert ? e + 1 : nvert - 1;
        const double a0 = V[3 * e], a1 = V[3 * e + 1], a2 = V[3 * e + 2], b0 = V[3 * f], b1 = V[3 * f + 1], b2 = V[3 * f + 2];
        const double dx = b0 - a0, dy = b1 - a1, dz = b2 - a2;
#pragma unroll
        for (int q = 0; q < N; ++q) {
          const bool b = seg_near(x[q] - a0, y[q] - a1, z[q] - a2, x[q] - b0, y[q] - b1, z[q] - b2, dx, dy, dz, re2);
          in |= (b ? 1u : 0u) << q;
        }
      }
    } break;
    default: break;
  }
  return in & gate;
}

// POLY = false: every record but the polyhedra, from no owner.  POLY = true: the polyhedron records alone, from the owners the first
// launch left in a.out (priority of an owner: its record's); the same tile, point map and single writer.
template <int PASS, bool POLY = false>
__global__ __launch_bounds__(VX_BLOCK) void k_voxel(const VoxArgs a) {
  using M = PtMap<PASS>;
  constexpr int N = M::N;
  constexpr int NOUT = PASS == PASS_CELL ? VX_PTS : 3 * VX_PTS;
  __shared__ unsigned long long s_tab[VX_CHUNK * VX_WORDS];
  __shared__ double s_tri[POLY ? VX_TRI_CHUNK * 9 : 1];           // the triangles of a chunk whose gate meets this tile
  __shared__ int s_cnt[VX_BLOCK / 64];

  // point counts of this pass and the block's tile
  const int px = PASS == PASS_CELL ? a.nx - 1 : a.nx, py = PASS == PASS_CELL ? a.ny - 1 : a.ny;
  const int pz = PASS == PASS_CELL ? a.nz - 1 : a.nz;
  const int tx = threadIdx.x % VX_TX, ty = threadIdx.x / VX_TX;
  const int bx0 = blockIdx.x * (VX_TX * VX_PTS), by0 = blockIdx.y * VX_TY, k = blockIdx.z;
  const int i0 = bx0 + tx * VX_PTS, j = by0 + ty;
  const int ext = PASS == PASS_EDGE ? 1 : 0;                      // the edge pass reads one node beyond the tile
  const int tx1 = min(bx0 + VX_TX * VX_PTS - 1 + ext, px - 1), ty1 = min(by0 + VX_TY - 1 + ext, py - 1), tz1 = min(k + ext, pz - 1);

  // coordinates (indices clamped to the grid: a clamped point is never inside an index box at its own index)
  const double* lx = a.lines;
  const double* ly = a.lines + a.nx;
  const double* lz = a.lines + a.nx + a.ny;
  double xs[VX_PTS + 1], ys[2], zs[2];
#pragma unroll
  for (int q = 0; q < VX_PTS + 1; ++q) {
    const int i = min(i0 + q, px - 1);
    xs[q] = PASS == PASS_CELL ? 0.5 * (lx[i] + lx[i + 1]) : lx[i];
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int jj = min(j + q, py - 1), kk = min(k + q, pz - 1);
    ys[q] = PASS == PASS_CELL ? 0.5 * (ly[jj] + ly[jj + 1]) : ly[jj];
    zs[q] = PASS == PASS_CELL ? 0.5 * (lz[kk] + lz[kk + 1]) : lz[kk];
  }
  double wx[N], wy[N], wz[N];
#pragma unroll
  for (int q = 0; q < N; ++q) { wx[q] = xs[M::xi(q)]; wy[q] = ys[M::yi(q)]; wz[q] = zs[M::zi(q)]; }

  int best[NOUT], own[NOUT];
#pragma unroll
  for (int q = 0; q < NOUT; ++q) { best[q] = INT32_MIN; own[q] = -1; }
  double cx[2] = {0.0, 0.0}, cy[2] = {0.0, 0.0}, cz[2] = {0.0, 0.0};   // POLY: the tile's first and last coordinate per axis (block-uniform);
  if constexpr (POLY) {                                              // the lines increase, so every point of the tile lies between them
    const int ix[2] = {bx0, tx1}, iy[2] = {by0, ty1}, iz[2] = {k, tz1};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      cx[q] = PASS == PASS_CELL ? 0.5 * (lx[ix[q]] + lx[ix[q] + 1]) : lx[ix[q]];
      cy[q] = PASS == PASS_CELL ? 0.5 * (ly[iy[q]] + ly[iy[q] + 1]) : ly[iy[q]];
      cz[q] = PASS == PASS_CELL ? 0.5 * (lz[iz[q]] + lz[iz[q] + 1]) : lz[iz[q]];
    }
    if (j < py) {
#pragma unroll
      for (int q = 0; q < NOUT; ++q) {
        if (i0 + q % VX_PTS >= px) continue;
        const size_t at = (size_t)(q / VX_PTS) * ((size_t)px * (size_t)py * (size_t)pz) + ((size_t)k * (size_t)py + (size_t)j) * (size_t)px + (size_t)(i0 + q % VX_PTS);
        own[q] = a.out[at];
        best[q] = own[q] >= 0 ? a.table[own[q]].priority : INT32_MIN;
      }
    }
  }

  for (int c0 = 0; c0 < a.nprim; c0 += VX_CHUNK) {
    const int cn = min(VX_CHUNK, a.nprim - c0);
    __syncthreads();                                              // the previous chunk is no longer read
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(a.table + c0);
    for (int w = threadIdx.x; w < cn * VX_WORDS; w += VX_BLOCK) s_tab[w] = src[w];
    __syncthreads();
    for (int p = 0; p < cn; ++p) {
      const fdtd_voxel_prim* r = reinterpret_cast<const fdtd_voxel_prim*>(s_tab + p * VX_WORDS);
      const int role = __builtin_amdgcn_readfirstlane(r->role);
      if (role != (PASS == PASS_CELL ? FDTD_VOXEL_MATERIAL : FDTD_VOXEL_METAL)) continue;
      const int32_t* box = PASS == PASS_CELL ? r->cbox : r->nbox;
      const int b0 = __builtin_amdgcn_readfirstlane(box[0]), b1 = __builtin_amdgcn_readfirstlane(box[1]);
      const int b2 = __builtin_amdgcn_readfirstlane(box[2]), b3 = __builtin_amdgcn_readfirstlane(box[3]);
      const int b4 = __builtin_amdgcn_readfirstlane(box[4]), b5 = __builtin_amdgcn_readfirstlane(box[5]);
      if (b3 < bx0 || b0 > tx1 || b4 < by0 || b1 > ty1 || b5 < k || b2 > tz1) continue;   // misses the tile: block-uniform
      const int type = __builtin_amdgcn_readfirstlane(r->type);
      if constexpr (POLY) {
        if (type != FDTD_VOXEL_POLYHEDRON) continue;              // the other launch holds no polyhedron: vx_test<N, false> gives it no point
      }
      const int prio = __builtin_amdgcn_readfirstlane(r->priority);
      const int norm_dir = __builtin_amdgcn_readfirstlane(r->norm_dir);
      const int vert0 = __builtin_amdgcn_readfirstlane(r->vert0), nvert = __builtin_amdgcn_readfirstlane(r->nvert);
      const bool has_matrix = __builtin_amdgcn_readfirstlane(r->has_matrix) != 0;
      unsigned gate = 0u;
#pragma unroll
      for (int q = 0; q < N; ++q) {
        const int i = i0 + M::xi(q), jj = j + M::yi(q), kk = k + M::zi(q);
        const bool g = i >= b0 && i <= b3 && jj >= b1 && jj <= b4 && kk >= b2 && kk <= b5;
        gate |= (g ? 1u : 0u) << q;
      }
      unsigned in;
      if constexpr (POLY) {
        // The record's triangles in chunks of one per thread: a thread tests its triangle's gate against the tile's (y, z) range in the
        // record's frame (each local coordinate is monotone in every world coordinate, so the tile's eight corners bound it); the
        // triangles that meet the tile are packed into LDS (ballot + prefix count, no atomics), and every thread runs those alone.
        // The order of the triangles does not matter: parity is an XOR, near an OR.
        double x[N], y[N], z[N];
        double Ylo = cy[0], Yhi = cy[1], Zlo = cz[0], Zhi = cz[1];
        if (has_matrix) {
          const double m0 = r->m[0], m1 = r->m[1], m2 = r->m[2], m3 = r->m[3], m4 = r->m[4], m5 = r->m[5], m6 = r->m[6], m7 = r->m[7],
                       m8 = r->m[8], m9 = r->m[9], m10 = r->m[10], m11 = r->m[11];
#pragma unroll
          for (int q = 0; q < N; ++q) {
            x[q] = ((m0 * wx[q] + m1 * wy[q]) + m2 * wz[q]) + m3;
            y[q] = ((m4 * wx[q] + m5 * wy[q]) + m6 * wz[q]) + m7;
            z[q] = ((m8 * wx[q] + m9 * wy[q]) + m10 * wz[q]) + m11;
          }
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const double X = cx[q & 1], Y = cy[(q >> 1) & 1], Z = cz[q >> 2];
            const double yy = ((m4 * X + m5 * Y) + m6 * Z) + m7, zz = ((m8 * X + m9 * Y) + m10 * Z) + m11;
            Ylo = (q == 0 || yy < Ylo) ? yy : Ylo; Yhi = (q == 0 || yy > Yhi) ? yy : Yhi;
            Zlo = (q == 0 || zz < Zlo) ? zz : Zlo; Zhi = (q == 0 || zz > Zhi) ? zz : Zhi;
          }
        } else {
#pragma unroll
          for (int q = 0; q < N; ++q) { x[q] = wx[q]; y[q] = wy[q]; z[q] = wz[q]; }
        }
        unsigned par = 0u, near = 0u;
        const int ntri = nvert / 3;
        const double* V = a.verts + vert0;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int t0 = 0; t0 < ntri; t0 += VX_TRI_CHUNK) {
          __syncthreads();                                          // the previous chunk's triangles are no longer read
          const int t = t0 + (int)threadIdx.x;
          double T[9];
          bool keep = false;
          if (t < ntri) {
#pragma unroll
            for (int q = 0; q < 9; ++q) T[q] = V[9 * (size_t)t + q];
            double y0, y1, z0, z1;
            tri_gate(T, 2.0 * a.tol, y0, y1, z0, z1);
            keep = !(Yhi < y0 || Ylo > y1 || Zhi < z0 || Zlo > z1);
          }
          const unsigned long long m = __ballot(keep);
          if (lane == 0) s_cnt[wave] = __popcll(m);
          __syncthreads();
          int base = 0, total = 0;
#pragma unroll
          for (int w = 0; w < VX_BLOCK / 64; ++w) { const int c = s_cnt[w]; base += w < wave ? c : 0; total += c; }
          if (keep) {
            const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
#pragma unroll
            for (int q = 0; q < 9; ++q) s_tri[9 * pos + q] = T[q];
          }
          __syncthreads();
          vx_tris<N>(s_tri, total, has_matrix, a.tol, x, y, z, gate, par, near);
        }
        in = (PASS == PASS_EDGE ? (par | near) : (par & ~near)) & gate;
      } else {
        in = vx_test<N, false>(r, type, PASS == PASS_EDGE, norm_dir, vert0, nvert, has_matrix, a.verts, a.tol, wx, wy, wz, gate);
      }
      const int idx = c0 + p;
      if (PASS == PASS_CELL) {
#pragma unroll
        for (int q = 0; q < VX_PTS; ++q) {
          const bool w = ((in >> q) & 1u) && vx_wins<POLY>(prio, idx, best[q], own[q]);
          best[q] = w ? prio : best[q];
          own[q] = w ? idx : own[q];
        }
      } else {
#pragma unroll
        for (int q = 0; q < VX_PTS; ++q) {
          const bool n0 = (in >> q) & 1u;
          const bool ex = n0 && ((in >> (q + 1)) & 1u), ey = n0 && ((in >> (q + 5)) & 1u), ez = n0 && ((in >> (q + 9)) & 1u);
          const bool w0 = ex && vx_wins<POLY>(prio, idx, best[q], own[q]), w1 = ey && vx_wins<POLY>(prio, idx, best[VX_PTS + q], own[VX_PTS + q]),
                     w2 = ez && vx_wins<POLY>(prio, idx, best[2 * VX_PTS + q], own[2 * VX_PTS + q]);
          best[q] = w0 ? prio : best[q];                       own[q] = w0 ? idx : own[q];
          best[VX_PTS + q] = w1 ? prio : best[VX_PTS + q];         own[VX_PTS + q] = w1 ? idx : own[VX_PTS + q];
          best[2 * VX_PTS + q] = w2 ? prio : best[2 * VX_PTS + q]; own[2 * VX_PTS + q] = w2 ? idx : own[2 * VX_PTS + q];
        }
      }
    }
  }

  // stores: int4 where the row length keeps every group of four 16-byte aligned (hipMalloc aligns the base)
  if (j >= py || i0 >= px) return;
  const size_t plane = (size_t)px * (size_t)py;
  const size_t row = ((size_t)k * (size_t)py + (size_t)j) * (size_t)px + (size_t)i0;
  const size_t comp_stride = plane * (size_t)pz;
  const bool wide = (px % 4 == 0) && (comp_stride % 4 == 0);     // block-uniform; i0 is a multiple of 4, so i0 + 3 < px
#pragma unroll
  for (int c = 0; c < (PASS == PASS_CELL ? 1 : 3); ++c) {
    int32_t* dst = a.out + (size_t)c * comp_stride + row;
    if (wide) {
      *reinterpret_cast<int4*>(dst) = make_int4(own[c * VX_PTS], own[c * VX_PTS + 1], own[c * VX_PTS + 2], own[c * VX_PTS + 3]);
    } else {
#pragma unroll
      for (int q = 0; q < VX_PTS; ++q)
        if (i0 + q < px) dst[q] = own[c * VX_PTS + q];
    }
  }
}
// ---- voxel maps (include/fdtd_hip_voxel.h: fdtd_voxelize_maps; discmaterial.lookup_spec is the same text in numpy) ---------------------
// One further launch over the records that delimit a voxel map, on k_voxel's tile and point map: it starts from the owners the earlier
// launches stored (as the polyhedron launch does, vx_wins<true>), tests the record's own predicate through vx_test, and for a cell the
// record would win looks its centre up in the map: three binary searches, every result range-checked, the linear index in 64 bits,
// one byte load.  Nothing is indexed by the byte.  Owner and voxel index have one writer each and are always written.
struct VxMapDev {
  double m[12];
  const double* lines[3];
  const uint8_t* data;
  int n[3];
  int use_bg;
};
struct MapArgs {
  VoxArgs v;                  // table: every record with its own index box; out: the owners of the earlier launches
  const int32_t* rec_map;     // per record: 0 none, m + 1
  const VxMapDev* maps;
  int32_t* vox;               // [nz-1][ny-1][nx-1]
};

// (the number of t with L[t] <= q) - 1 over the n increasing lines L: -1 .. n - 1; a NaN compares false everywhere: -1
__device__ __forceinline__ int vx_line_index(const double* __restrict__ L, const int n, const double q) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;                                  // 0 <= mid <= n - 1
    if (L[mid] <= q) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

__global__ __launch_bounds__(VX_BLOCK) void k_voxel_map(const MapArgs ma) {
  using M = PtMap<PASS_CELL>;
  constexpr int N = M::N;
  const VoxArgs& a = ma.v;
  __shared__ unsigned long long s_tab[VX_CHUNK * VX_WORDS];
  __shared__ int s_map[VX_CHUNK];

  const int px = a.nx - 1, py = a.ny - 1;
  const int tx = threadIdx.x % VX_TX, ty = threadIdx.x / VX_TX;
  const int bx0 = blockIdx.x * (VX_TX * VX_PTS), by0 = blockIdx.y * VX_TY, k = blockIdx.z;   // k < nz - 1: the grid's z extent
  const int i0 = bx0 + tx * VX_PTS, j = by0 + ty;
  const int tx1 = min(bx0 + VX_TX * VX_PTS - 1, px - 1), ty1 = min(by0 + VX_TY - 1, py - 1);

  // cell centres (indices clamped to the grid: a clamped point is never inside an index box at its own index)
  const double* lx = a.lines;
  const double* ly = a.lines + a.nx;
  const double* lz = a.lines + a.nx + a.ny;
  double wx[N], wy[N], wz[N];
  {
    const int jj = min(j, py - 1);
    const double yc = 0.5 * (ly[jj] + ly[jj + 1]), zc = 0.5 * (lz[k] + lz[k + 1]);
#pragma unroll
    for (int q = 0; q < N; ++q) {
      const int i = min(i0 + q, px - 1);
      wx[q] = 0.5 * (lx[i] + lx[i + 1]); wy[q] = yc; wz[q] = zc;
    }
  }
  const bool live = j < py && i0 < px;
  const size_t row = ((size_t)k * (size_t)py + (size_t)min(j, py - 1)) * (size_t)px + (size_t)min(i0, px - 1);
  int best[VX_PTS], own[VX_PTS], vox[VX_PTS];
#pragma unroll
  for (int q = 0; q < VX_PTS; ++q) {
    best[q] = INT32_MIN; own[q] = -1; vox[q] = -1;
    if (live && i0 + q < px) {
      own[q] = a.out[row + q];
      best[q] = own[q] >= 0 ? a.table[own[q]].priority : INT32_MIN;
    }
  }

  for (int c0 = 0; c0 < a.nprim; c0 += VX_CHUNK) {
    const int cn = min(VX_CHUNK, a.nprim - c0);
    __syncthreads();                                              // the previous chunk is no longer read
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(a.table + c0);
    for (int w = threadIdx.x; w < cn * VX_WORDS; w += VX_BLOCK) s_tab[w] = src[w];
    if ((int)threadIdx.x < cn) s_map[threadIdx.x] = ma.rec_map[c0 + threadIdx.x];
    __syncthreads();
    for (int p = 0; p < cn; ++p) {
      const int mi = __builtin_amdgcn_readfirstlane(s_map[p]);
      if (mi == 0) continue;                                      // the earlier launches took this record
      const fdtd_voxel_prim* r = reinterpret_cast<const fdtd_voxel_prim*>(s_tab + p * VX_WORDS);
      const int b0 = __builtin_amdgcn_readfirstlane(r->cbox[0]), b1 = __builtin_amdgcn_readfirstlane(r->cbox[1]);
      const int b2 = __builtin_amdgcn_readfirstlane(r->cbox[2]), b3 = __builtin_amdgcn_readfirstlane(r->cbox[3]);
      const int b4 = __builtin_amdgcn_readfirstlane(r->cbox[4]), b5 = __builtin_amdgcn_readfirstlane(r->cbox[5]);
      if (b3 < bx0 || b0 > tx1 || b4 < by0 || b1 > ty1 || b5 < k || b2 > k) continue;     // misses the tile: block-uniform
      const int type = __builtin_amdgcn_readfirstlane(r->type);
      const int prio = __builtin_amdgcn_readfirstlane(r->priority);
      const int norm_dir = __builtin_amdgcn_readfirstlane(r->norm_dir);
      const int vert0 = __builtin_amdgcn_readfirstlane(r->vert0), nvert = __builtin_amdgcn_readfirstlane(r->nvert);
      const bool has_matrix = __builtin_amdgcn_readfirstlane(r->has_matrix) != 0;
      const int idx = c0 + p;
      unsigned gate = 0u;
#pragma unroll
      for (int q = 0; q < N; ++q) {
        const int i = i0 + q;
        const bool g = i >= b0 && i <= b3 && j >= b1 && j <= b4 && k >= b2 && k <= b5 && vx_wins<true>(prio, idx, best[q], own[q]);
        gate |= (g ? 1u : 0u) << q;                               // a cell the record cannot win needs neither test
      }
      const unsigned in = vx_test<N, false>(r, type, false, norm_dir, vert0, nvert, has_matrix, a.verts, a.tol, wx, wy, wz, gate);
      if (in == 0u) continue;
      const VxMapDev* mp = ma.maps + (mi - 1);                    // host: 1 <= mi <= nmaps
      const double m0 = mp->m[0], m1 = mp->m[1], m2 = mp->m[2], m3 = mp->m[3], m4 = mp->m[4], m5 = mp->m[5], m6 = mp->m[6], m7 = mp->m[7],
                   m8 = mp->m[8], m9 = mp->m[9], m10 = mp->m[10], m11 = mp->m[11];
      const int n0 = mp->n[0], n1 = mp->n[1], n2 = mp->n[2];
      const bool bg = mp->use_bg != 0;
#pragma unroll
      for (int q = 0; q < N; ++q) {
        if (!((in >> q) & 1u)) continue;
        const double qx = ((m0 * wx[q] + m1 * wy[q]) + m2 * wz[q]) + m3;
        const double qy = ((m4 * wx[q] + m5 * wy[q]) + m6 * wz[q]) + m7;
        const double qz = ((m8 * wx[q] + m9 * wy[q]) + m10 * wz[q]) + m11;
        const int ix = vx_line_index(mp->lines[0], n0, qx);
        if (ix < 0 || ix > n0 - 2) continue;
        const int iy = vx_line_index(mp->lines[1], n1, qy);
        if (iy < 0 || iy > n1 - 2) continue;
        const int iz = vx_line_index(mp->lines[2], n2, qz);
        if (iz < 0 || iz > n2 - 2) continue;
        const long long lin = ((long long)iz * (long long)(n1 - 1) + (long long)iy) * (long long)(n0 - 1) + (long long)ix;
        const uint8_t v = mp->data[lin];                          // 0 <= lin < (n0-1)(n1-1)(n2-1) == the data's length (host) <= 2^31 - 1
        if (v == 0 && !bg) continue;                              // the background voxel is transparent
        best[q] = prio; own[q] = idx; vox[q] = (int)lin;
      }
    }
  }

  if (!live) return;
  const bool wide = px % 4 == 0;                                  // block-uniform; i0 and then row are multiples of 4 (hipMalloc aligns the base)
  if (wide) {
    *reinterpret_cast<int4*>(a.out + row) = make_int4(own[0], own[1], own[2], own[3]);
    *reinterpret_cast<int4*>(ma.vox + row) = make_int4(vox[0], vox[1], vox[2], vox[3]);
  } else {
#pragma unroll
    for (int q = 0; q < VX_PTS; ++q)
      if (i0 + q < px) { a.out[row + q] = own[q]; ma.vox[row + q] = vox[q]; }
  }
}

// ---- conformal fractions (include/fdtd_hip_conformal.h, conformal.fractions_spec) -----------------------------------------------
// Both kernels call vx_test<1> on the records in global memory: the inside predicates are the rasteriser's own text, so a node's
// or a bisection point's verdict has the bits of primitives._inside.  A cut edge costs nbisect * (records whose node box holds one
// of its two nodes) predicates; the cut edges are a surface, a few per cent of the grid at most.
struct FracArgs {
  int nx, ny, nz;
  const double* lines;
  int nprim;
  const fdtd_voxel_prim* table;
  const double* verts;
  double tol, snap;
  int nbisect;
  uint8_t* node_in;          // [nz][ny][nx]
  long long ncut;
  const uint8_t* code;       // comp | flip << 2
  const long long* idx;
  double* f;
};

__device__ __forceinline__ bool vx_holds(const fdtd_voxel_prim* r, const double* verts, const double tol, const double x, const double y,
                                         const double z) {
  const double wx[1] = {x}, wy[1] = {y}, wz[1] = {z};
  return vx_test<1>(r, r->type, true, r->norm_dir, r->vert0, r->nvert, r->has_matrix != 0, verts, tol, wx, wy, wz, 1u) != 0u;
}
__device__ __forceinline__ bool vx_in_box(const fdtd_voxel_prim* r, const int i, const int j, const int k) {
  return i >= r->nbox[0] && i <= r->nbox[3] && j >= r->nbox[1] && j <= r->nbox[4] && k >= r->nbox[2] && k <= r->nbox[5];
}

__global__ __launch_bounds__(VX_BLOCK) void k_node_in(const FracArgs a) {
  const long long q = (long long)blockIdx.x * VX_BLOCK + threadIdx.x;
  const long long nn = (long long)a.nx * a.ny * a.nz;
  if (q >= nn) return;
  const int i = (int)(q % a.nx), j = (int)((q / a.nx) % a.ny), k = (int)(q / ((long long)a.nx * a.ny));
  const double x = a.lines[i], y = a.lines[a.nx + j], z = a.lines[a.nx + a.ny + k];
  bool in = false;
  for (int p = 0; p < a.nprim; ++p) {
    const fdtd_voxel_prim* r = a.table + p;
    if (!vx_in_box(r, i, j, k)) continue;
    in = in || vx_holds(r, a.verts, a.tol, x, y, z);
  }
  a.node_in[q] = in ? 1 : 0;
}

__global__ __launch_bounds__(VX_BLOCK) void k_fractions(const FracArgs a) {
  const long long e = (long long)blockIdx.x * VX_BLOCK + threadIdx.x;
  if (e >= a.ncut) return;
  const int c = a.code[e] & 3;
  const bool flip = (a.code[e] >> 2) & 1;
  const long long g = a.idx[e];
  const int i = (int)(g % a.nx), j = (int)((g / a.nx) % a.ny), k = (int)(g / ((long long)a.nx * a.ny));
  const int i1 = i + (c == 0 ? 1 : 0), j1 = j + (c == 1 ? 1 : 0), k1 = k + (c == 2 ? 1 : 0);
  double p[3] = {a.lines[i], a.lines[a.nx + j], a.lines[a.nx + a.ny + k]};
  const double lower = p[c];
  const double upper = c == 0 ? a.lines[i1] : c == 1 ? a.lines[a.nx + j1] : a.lines[a.nx + a.ny + k1];
  const double x_in = flip ? upper : lower, x_out = flip ? lower : upper;
  const double d = x_out - x_in;
  double ta = 0.0, tb = 1.0;
  for (int it = 0; it < a.nbisect; ++it) {
    const double tm = 0.5 * (ta + tb);
    const double x = x_in + tm * d;
    const double px = c == 0 ? x : p[0], py = c == 1 ? x : p[1], pz = c == 2 ? x : p[2];
    bool in = false;
    for (int q = 0; q < a.nprim && !in; ++q) {
      const fdtd_voxel_prim* r = a.table + q;
      if (!vx_in_box(r, i, j, k) && !vx_in_box(r, i1, j1, k1)) continue;
      in = vx_holds(r, a.verts, a.tol, px, py, pz);
    }
    ta = in ? tm : ta;
    tb = in ? tb : tm;
  }
  const double len = d < 0.0 ? -d : d;
  a.f[e] = ta * len <= a.snap ? 1.0 : 1.0 - ta;
}

// The host part of fdtd_voxelize: validates the table and copies it to out[nprim] with its index boxes clipped to the grid.
int vx_check_table(int nx, int ny, int nz, int nprim, const void* table, int nvert, fdtd_voxel_prim* out) {
  if (nx < 2 || ny < 2 || nz < 2 || nprim < 0 || nvert < 0 || (nprim > 0 && (!table || !out)))
    return fdtd_fail(nullptr, FDTD_E_ARG, "bad voxelize argument");
  const int nn[3] = {nx, ny, nz};
  for (int p = 0; p < nprim; ++p) {
    fdtd_voxel_prim r;
    memcpy(&r, (const char*)table + (size_t)p * sizeof(r), sizeof(r));
    if (r.type < 0 || r.type >= FDTD_VOXEL_NTYPES || (r.role != FDTD_VOXEL_MATERIAL && r.role != FDTD_VOXEL_METAL))
      return fdtd_fail(nullptr, FDTD_E_ARG, "voxelize: record %d has type %d, role %d", p, r.type, r.role);
    const bool poly = r.type == FDTD_VOXEL_POLYGON || r.type == FDTD_VOXEL_LINPOLY, wire = r.type == FDTD_VOXEL_WIRE;
    const bool mesh = r.type == FDTD_VOXEL_POLYHEDRON;                 // nvert = 3 * ntri points of three doubles
    if (poly || wire || mesh) {
      const long long need = (long long)r.vert0 + (long long)(poly ? 2 : 3) * (long long)r.nvert;
      if (r.vert0 < 0 || r.nvert < 1 || need > (long long)nvert || (mesh && r.nvert % 3 != 0))
        return fdtd_fail(nullptr, FDTD_E_ARG, "voxelize: record %d reads vertices %d + %d of %d", p, r.vert0, r.nvert, nvert);
      if (poly && (r.norm_dir < 0 || r.norm_dir > 2))
        return fdtd_fail(nullptr, FDTD_E_ARG, "voxelize: record %d has norm_dir %d", p, r.norm_dir);
    }
    for (int ax = 0; ax < 3; ++ax) {                              // clip the index boxes to the grid
      if (r.cbox[ax] < 0) r.cbox[ax] = 0;
      if (r.cbox[3 + ax] > nn[ax] - 2) r.cbox[3 + ax] = nn[ax] - 2;
      if (r.nbox[ax] < 0) r.nbox[ax] = 0;
      if (r.nbox[3 + ax] > nn[ax] - 1) r.nbox[3 + ax] = nn[ax] - 1;
    }
    out[p] = r;
  }
  return FDTD_OK;
}

// The host part of fdtd_voxelize_maps: rec_map and the maps themselves.  After it no lookup can leave a map's lines or data.
int vx_check_maps(int nprim, const fdtd_voxel_prim* tab, const int32_t* rec_map, int nmaps, const fdtd_voxel_map* maps) {
  if (nmaps < 0 || nmaps > FDTD_VOXEL_MAX_MAPS || (nmaps > 0 && (!maps || (nprim > 0 && !rec_map))))
    return fdtd_fail(nullptr, FDTD_E_ARG, "voxelize: %d voxel maps (0..%d, with rec_map and maps)", nmaps, (int)FDTD_VOXEL_MAX_MAPS);
  for (int m = 0; m < nmaps; ++m) {
    const fdtd_voxel_map& v = maps[m];
    long long nvox = 1;
    for (int ax = 0; ax < 3; ++ax) {
      if (v.n[ax] < 2 || !v.lines[ax]) return fdtd_fail(nullptr, FDTD_E_ARG, "voxelize: map %d has %d lines on axis %d (>= 2)", m, v.n[ax], ax);
      for (int t = 1; t < v.n[ax]; ++t)
        if (!(v.lines[ax][t] > v.lines[ax][t - 1])) return fdtd_fail(nullptr, FDTD_E_ARG, "voxelize: map %d: the lines of axis %d do not increase at %d", m, ax, t);
      nvox *= (long long)(v.n[ax] - 1);                           // each factor < 2^31: checked after every product
      if (nvox > (long long)INT32_MAX) return fdtd_fail(nullptr, FDTD_E_ARG, "voxelize: map %d has more than 2^31 - 1 voxels", m);
    }
    if (!v.data || (long long)v.ndata != nvox)
      return fdtd_fail(nullptr, FDTD_E_ARG, "voxelize: map %d: data of %lld bytes for %lld voxels", m, (long long)v.ndata, nvox);
  }
  for (int p = 0; p < nprim && nmaps > 0; ++p) {
    if (rec_map[p] < 0 || rec_map[p] > nmaps) return fdtd_fail(nullptr, FDTD_E_ARG, "voxelize: record %d refers to map %d of %d", p, rec_map[p], nmaps);
    if (rec_map[p] != 0 && (tab[p].role != FDTD_VOXEL_MATERIAL || tab[p].type == FDTD_VOXEL_POLYHEDRON))
      return fdtd_fail(nullptr, FDTD_E_ARG, "voxelize: record %d delimits a voxel map: a material that is no polyhedron expected", p);
  }
  return FDTD_OK;
}
}  // namespace

static int vx_run(int device, int nx, int ny, int nz, const double* lines, int nprim, const void* table, int nvert, const double* verts,
                  double tol, int32_t* cell_owner, int32_t* edge_owner, const int32_t* rec_map, int nmaps, const fdtd_voxel_map* maps,
                  int32_t* cell_voxel) {
  if (!lines || (nvert > 0 && !verts) || !(tol >= 0.0) || (cell_voxel && !cell_owner)) return fdtd_fail(nullptr, FDTD_E_ARG, "bad voxelize argument");
  std::vector<fdtd_voxel_prim> tab;
  try {
    tab.resize((size_t)(nprim > 0 ? nprim : 0));
  } catch (...) {
    return fdtd_fail(nullptr, FDTD_E_NOMEM, "voxelize: no host memory for %d records", nprim);
  }
  int rc = vx_check_table(nx, ny, nz, nprim, table, nvert, tab.data());
  if (rc != FDTD_OK) return rc;
  rc = vx_check_maps(nprim, tab.data(), rec_map, nmaps, maps);
  if (rc != FDTD_OK) return rc;
  const size_t ncell = (size_t)(nx - 1) * (size_t)(ny - 1) * (size_t)(nz - 1), nedge = 3 * (size_t)nx * (size_t)ny * (size_t)nz;
  // The records that delimit a voxel map leave the launches below (an empty index box misses every tile) and take k_voxel_map, which
  // reads them from `full`.
  std::vector<fdtd_voxel_prim> full;
  bool mapped = false;
  for (int p = 0; p < nprim && nmaps > 0; ++p) mapped = mapped || rec_map[p] != 0;
  if (mapped) {
    try {
      full = tab;
    } catch (...) {
      return fdtd_fail(nullptr, FDTD_E_NOMEM, "voxelize: no host memory for %d records", nprim);
    }
    const int32_t none[6] = {0, 0, 0, -1, -1, -1};
    for (int p = 0; p < nprim; ++p)
      if (rec_map[p] != 0) memcpy(tab[p].cbox, none, sizeof(none));
  }
  if (cell_voxel && !mapped) for (size_t q = 0; q < ncell; ++q) cell_voxel[q] = -1;
  if (nprim == 0) {                                               // nothing drawn: no device work
    if (cell_owner) for (size_t q = 0; q < ncell; ++q) cell_owner[q] = -1;
    if (edge_owner) for (size_t q = 0; q < nedge; ++q) edge_owner[q] = -1;
    return FDTD_OK;
  }
  if (!cell_owner && !edge_owner) return FDTD_OK;
  HIPCK(nullptr, hipSetDevice(device));
  double *d_lines = nullptr, *d_verts = nullptr;
  fdtd_voxel_prim* d_tab = nullptr;
  int32_t *d_cell = nullptr, *d_edge = nullptr;
  // voxel maps (cell pass with mapped records only): the full table, rec_map, the maps' descriptors, per map its lines and voxels
  const bool run_maps = mapped && cell_owner;
  fdtd_voxel_prim* d_full = nullptr;
  int32_t *d_recmap = nullptr, *d_vox = nullptr;
  VxMapDev* d_maps = nullptr;
  double* d_mlines[FDTD_VOXEL_MAX_MAPS] = {nullptr, nullptr, nullptr, nullptr};
  uint8_t* d_mdata[FDTD_VOXEL_MAX_MAPS] = {nullptr, nullptr, nullptr, nullptr};
  const size_t nl = (size_t)nx + (size_t)ny + (size_t)nz;
#define VX(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess && rc == FDTD_OK) rc = fdtd_fail(nullptr, e_ == hipErrorOutOfMemory ? FDTD_E_NOMEM : FDTD_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); } while (0)
  VX(hipMalloc(&d_lines, nl * sizeof(double)));
  VX(hipMalloc(&d_verts, (size_t)(nvert > 0 ? nvert : 1) * sizeof(double)));
  VX(hipMalloc(&d_tab, (size_t)nprim * sizeof(fdtd_voxel_prim)));
  if (cell_owner) VX(hipMalloc(&d_cell, ncell * sizeof(int32_t)));
  if (edge_owner) VX(hipMalloc(&d_edge, nedge * sizeof(int32_t)));
  if (run_maps) {
    VX(hipMalloc(&d_full, (size_t)nprim * sizeof(fdtd_voxel_prim)));
    VX(hipMalloc(&d_recmap, (size_t)nprim * sizeof(int32_t)));
    VX(hipMalloc(&d_maps, (size_t)nmaps * sizeof(VxMapDev)));
    VX(hipMalloc(&d_vox, ncell * sizeof(int32_t)));
    for (int m = 0; m < nmaps; ++m) {
      VX(hipMalloc(&d_mlines[m], ((size_t)maps[m].n[0] + (size_t)maps[m].n[1] + (size_t)maps[m].n[2]) * sizeof(double)));
      VX(hipMalloc(&d_mdata[m], (size_t)maps[m].ndata));
    }
  }
  if (rc == FDTD_OK) {
    VX(hipMemcpy(d_lines, lines, nl * sizeof(double), hipMemcpyHostToDevice));
    if (nvert > 0) VX(hipMemcpy(d_verts, verts, (size_t)nvert * sizeof(double), hipMemcpyHostToDevice));
    VX(hipMemcpy(d_tab, tab.data(), (size_t)nprim * sizeof(fdtd_voxel_prim), hipMemcpyHostToDevice));
  }
  if (rc == FDTD_OK && run_maps) {
    VxMapDev dev[FDTD_VOXEL_MAX_MAPS];
    for (int m = 0; m < nmaps; ++m) {
      const fdtd_voxel_map& v = maps[m];
      memcpy(dev[m].m, v.m, sizeof(v.m));
      size_t off = 0;
      for (int ax = 0; ax < 3; ++ax) {
        VX(hipMemcpy(d_mlines[m] + off, v.lines[ax], (size_t)v.n[ax] * sizeof(double), hipMemcpyHostToDevice));
        dev[m].lines[ax] = d_mlines[m] + off;
        dev[m].n[ax] = v.n[ax];
        off += (size_t)v.n[ax];
      }
      VX(hipMemcpy(d_mdata[m], v.data, (size_t)v.ndata, hipMemcpyHostToDevice));
      dev[m].data = d_mdata[m];
      dev[m].use_bg = v.use_db_background != 0 ? 1 : 0;
    }
    VX(hipMemcpy(d_maps, dev, (size_t)nmaps * sizeof(VxMapDev), hipMemcpyHostToDevice));
    VX(hipMemcpy(d_full, full.data(), (size_t)nprim * sizeof(fdtd_voxel_prim), hipMemcpyHostToDevice));
    VX(hipMemcpy(d_recmap, rec_map, (size_t)nprim * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  if (rc == FDTD_OK) {
    VoxArgs a{nx, ny, nz, d_lines, nprim, d_tab, d_verts, tol, nullptr};
    const int per_x = VX_TX * VX_PTS;
    bool mesh[2] = {false, false};                               // a polyhedron among the materials / the metals: its own launch
    for (int p = 0; p < nprim; ++p)
      if (tab[p].type == FDTD_VOXEL_POLYHEDRON) mesh[tab[p].role == FDTD_VOXEL_METAL ? 1 : 0] = true;
    if (cell_owner) {
      a.out = d_cell;
      hipLaunchKernelGGL(k_voxel<PASS_CELL>, dim3((nx - 1 + per_x - 1) / per_x, (ny - 1 + VX_TY - 1) / VX_TY, nz - 1), dim3(VX_BLOCK), 0, 0, a);
      if (mesh[0])
        hipLaunchKernelGGL((k_voxel<PASS_CELL, true>), dim3((nx - 1 + per_x - 1) / per_x, (ny - 1 + VX_TY - 1) / VX_TY, nz - 1), dim3(VX_BLOCK), 0, 0, a);
      if (run_maps) {                                             // same stream: after the owners of the launches above are stored
        MapArgs ma{a, d_recmap, d_maps, d_vox};
        ma.v.table = d_full;
        hipLaunchKernelGGL(k_voxel_map, dim3((nx - 1 + per_x - 1) / per_x, (ny - 1 + VX_TY - 1) / VX_TY, nz - 1), dim3(VX_BLOCK), 0, 0, ma);
      }
      VX(hipGetLastError());
    }
    if (edge_owner) {
      a.out = d_edge;
      hipLaunchKernelGGL(k_voxel<PASS_EDGE>, dim3((nx + per_x - 1) / per_x, (ny + VX_TY - 1) / VX_TY, nz), dim3(VX_BLOCK), 0, 0, a);
      if (mesh[1])
        hipLaunchKernelGGL((k_voxel<PASS_EDGE, true>), dim3((nx + per_x - 1) / per_x, (ny + VX_TY - 1) / VX_TY, nz), dim3(VX_BLOCK), 0, 0, a);
      VX(hipGetLastError());
    }
    VX(hipDeviceSynchronize());
    if (rc == FDTD_OK && cell_owner) VX(hipMemcpy(cell_owner, d_cell, ncell * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (rc == FDTD_OK && edge_owner) VX(hipMemcpy(edge_owner, d_edge, nedge * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (rc == FDTD_OK && run_maps && cell_voxel) VX(hipMemcpy(cell_voxel, d_vox, ncell * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
#undef VX
  hipFree(d_lines); hipFree(d_verts); hipFree(d_tab); hipFree(d_cell); hipFree(d_edge);
  hipFree(d_full); hipFree(d_recmap); hipFree(d_maps); hipFree(d_vox);
  for (int m = 0; m < FDTD_VOXEL_MAX_MAPS; ++m) { hipFree(d_mlines[m]); hipFree(d_mdata[m]); }
  return rc;
}
extern "C" int fdtd_voxelize(int device, int nx, int ny, int nz, const double* lines, int nprim, const void* table, int nvert,
                             const double* verts, double tol, int32_t* cell_owner, int32_t* edge_owner) {
  return vx_run(device, nx, ny, nz, lines, nprim, table, nvert, verts, tol, cell_owner, edge_owner, nullptr, 0, nullptr, nullptr);
}
extern "C" int fdtd_voxelize_maps(int device, int nx, int ny, int nz, const double* lines, int nprim, const void* table, int nvert,
                                  const double* verts, double tol, int32_t* cell_owner, int32_t* edge_owner, const int32_t* rec_map, int nmaps,
                                  const fdtd_voxel_map* maps, int32_t* cell_voxel) {
  return vx_run(device, nx, ny, nz, lines, nprim, table, nvert, verts, tol, cell_owner, edge_owner, rec_map, nmaps, maps, cell_voxel);
}
extern "C" int fdtd_voxel_fractions(int device, int nx, int ny, int nz, const double* lines, int nprim, const void* table, int nvert,
                                    const double* verts, double tol, double snap, int nbisect, uint8_t* node_in, int64_t ncut,
                                    const uint8_t* code, const int64_t* idx, double* f) {
  if (!lines || (nvert > 0 && !verts) || !(tol >= 0.0) || !(snap >= 0.0) || nbisect < 1 || nbisect > 60 || ncut < 0 ||
      (ncut > 0 && (!code || !idx || !f)))
    return fdtd_fail(nullptr, FDTD_E_ARG, "bad fractions argument");
  std::vector<fdtd_voxel_prim> tab;
  try {
    tab.resize((size_t)(nprim > 0 ? nprim : 0));
  } catch (...) {
    return fdtd_fail(nullptr, FDTD_E_NOMEM, "fractions: no host memory for %d records", nprim);
  }
  int rc = vx_check_table(nx, ny, nz, nprim, table, nvert, tab.data());
  if (rc != FDTD_OK) return rc;
  for (int p = 0; p < nprim; ++p)
    if (tab[p].role != FDTD_VOXEL_METAL) return fdtd_fail(nullptr, FDTD_E_ARG, "fractions: record %d is no metal", p);
  const long long nn = (long long)nx * ny * nz;
  for (int64_t e = 0; e < ncut; ++e) {                              // every edge inside the grid and existing
    const int c = code[e] & 3;
    const long long g = idx[e];
    if (c > 2 || code[e] > 7 || g < 0 || g >= nn) return fdtd_fail(nullptr, FDTD_E_ARG, "fractions: edge %lld out of range", (long long)e);
    const int pos[3] = {(int)(g % nx), (int)((g / nx) % ny), (int)(g / ((long long)nx * ny))};
    const int lim[3] = {nx, ny, nz};
    if (pos[c] >= lim[c] - 1) return fdtd_fail(nullptr, FDTD_E_ARG, "fractions: edge %lld does not exist", (long long)e);
  }
  if (nprim == 0) {                                                 // nothing drawn: no node inside, no edge cut
    if (node_in) memset(node_in, 0, (size_t)nn);
    for (int64_t e = 0; e < ncut; ++e) f[e] = 1.0;
    return FDTD_OK;
  }
  if (!node_in && ncut == 0) return FDTD_OK;
  HIPCK(nullptr, hipSetDevice(device));
  double *d_lines = nullptr, *d_verts = nullptr, *d_f = nullptr;
  fdtd_voxel_prim* d_tab = nullptr;
  uint8_t *d_node = nullptr, *d_code = nullptr;
  long long* d_idx = nullptr;
  const size_t nl = (size_t)nx + (size_t)ny + (size_t)nz;
#define VX(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess && rc == FDTD_OK) rc = fdtd_fail(nullptr, e_ == hipErrorOutOfMemory ? FDTD_E_NOMEM : FDTD_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); } while (0)
  VX(hipMalloc(&d_lines, nl * sizeof(double)));
  VX(hipMalloc(&d_verts, (size_t)(nvert > 0 ? nvert : 1) * sizeof(double)));
  VX(hipMalloc(&d_tab, (size_t)nprim * sizeof(fdtd_voxel_prim)));
  if (node_in) VX(hipMalloc(&d_node, (size_t)nn));
  if (ncut > 0) {
    VX(hipMalloc(&d_code, (size_t)ncut));
    VX(hipMalloc(&d_idx, (size_t)ncut * sizeof(long long)));
    VX(hipMalloc(&d_f, (size_t)ncut * sizeof(double)));
  }
  if (rc == FDTD_OK) {
    VX(hipMemcpy(d_lines, lines, nl * sizeof(double), hipMemcpyHostToDevice));
    if (nvert > 0) VX(hipMemcpy(d_verts, verts, (size_t)nvert * sizeof(double), hipMemcpyHostToDevice));
    VX(hipMemcpy(d_tab, tab.data(), (size_t)nprim * sizeof(fdtd_voxel_prim), hipMemcpyHostToDevice));
    if (ncut > 0) {
      VX(hipMemcpy(d_code, code, (size_t)ncut, hipMemcpyHostToDevice));
      VX(hipMemcpy(d_idx, idx, (size_t)ncut * sizeof(long long), hipMemcpyHostToDevice));
    }
  }
  if (rc == FDTD_OK) {
    FracArgs a{nx, ny, nz, d_lines, nprim, d_tab, d_verts, tol, snap, nbisect, d_node, (long long)ncut, d_code, d_idx, d_f};
    if (node_in) {
      hipLaunchKernelGGL(k_node_in, dim3((unsigned)((nn + VX_BLOCK - 1) / VX_BLOCK)), dim3(VX_BLOCK), 0, 0, a);
      VX(hipGetLastError());
    }
    if (ncut > 0) {
      hipLaunchKernelGGL(k_fractions, dim3((unsigned)((ncut + VX_BLOCK - 1) / VX_BLOCK)), dim3(VX_BLOCK), 0, 0, a);
      VX(hipGetLastError());
    }
    VX(hipDeviceSynchronize());
    if (rc == FDTD_OK && node_in) VX(hipMemcpy(node_in, d_node, (size_t)nn, hipMemcpyDeviceToHost));
    if (rc == FDTD_OK && ncut > 0) VX(hipMemcpy(f, d_f, (size_t)ncut * sizeof(double), hipMemcpyDeviceToHost));
  }
#undef VX
  hipFree(d_lines); hipFree(d_verts); hipFree(d_tab); hipFree(d_node); hipFree(d_code); hipFree(d_idx); hipFree(d_f);
  return rc;
}

// ---- sub-cell averaged dielectric surfaces (include/fdtd_hip_subcell.h, subcell.edges_spec) -------------------------------------------
// Pass A (k_sub_cells) owns the sub-voxel lattice: the lanes of a wave are the sub-voxels of one cell (nsub = 4: 64 lanes, one point
// each; nsub = 8: eight points a lane; nsub = 2: eight cells a wave), the record loop is wave-uniform (the records are read through a
// uniform pointer, a record whose grown cell box misses every cell of the wave is skipped by a ballot), and the predicate is vx_test,
// the rasteriser's own text.  Its first launch stores one uint16 per cell: the material of a cell whose sub-voxels all have one owner's,
// SUB_MIXED otherwise (a ballot).  The host numbers the mixed cells and lists the candidate edges (an edge with a mixed cell among its
// four, found from the mixed cells); the second launch stores the lattices of the mixed cells alone, compacted — the lattice of the whole grid is never held.
// Pass B (k_sub_edges), one thread per candidate edge, reads them and does the header's sums in the header's order.  Every output
// word has one writer; plain vector stores, no atomics.
#include <algorithm>

#include "../../include/fdtd_hip_subcell.h"

namespace {
constexpr uint16_t SUB_MIXED = 0xFFFF;

struct SubArgs {
  int nx, ny, nz;
  const double* lines;
  int nprim;
  const fdtd_voxel_prim* table;      // index boxes clipped to the grid (vx_check_table)
  const double* verts;
  double tol;
  int nsub, nprop;
  long long ncells;                  // the cells of this launch, >= 1
  const int32_t* cells;              // FILL: their flat cell indices; otherwise the launch covers cells 0 .. ncells - 1
  uint16_t* out;                     // per cell one code, or FILL: per cell nsub^3 materials, sub-voxel x fastest
};

template <int N, bool FILL>
__global__ __launch_bounds__(VX_BLOCK) void k_sub_cells(const SubArgs a) {
  const int nsub = a.nsub, pts = nsub * nsub * nsub;
  const int per_cell = pts / N;                                   // lanes of one cell: 8, 64, 64
  const int cpw = 64 / per_cell;                                  // cells of one wave: 8, 1, 1
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (VX_BLOCK / 64) + (threadIdx.x >> 6);
  const int g = lane / per_cell, sv0 = lane % per_cell;           // point q of this lane is sub-voxel sv0 + q * per_cell
  const long long w = wave * cpw + g;
  const bool valid = w < a.ncells;
  const long long wc = valid ? w : a.ncells - 1;                  // a lane beyond the end repeats the last cell and stores nothing
  const long long cell = FILL ? (long long)a.cells[wc] : wc;
  const int cx = a.nx - 1, cy = a.ny - 1, cz = a.nz - 1;
  const int i = (int)(cell % cx), j = (int)((cell / cx) % cy), k = (int)(cell / ((long long)cx * cy));   // 0 <= i, j, k <= n - 2
  const double* lx = a.lines;
  const double* ly = a.lines + a.nx;
  const double* lz = a.lines + a.nx + a.ny;
  const double inv = 1.0 / nsub;
  const double x0 = lx[i], dx = lx[i + 1] - lx[i], y0 = ly[j], dy = ly[j + 1] - ly[j], z0 = lz[k], dz = lz[k + 1] - lz[k];
  double wx[N], wy[N], wz[N];
#pragma unroll
  for (int q = 0; q < N; ++q) {
    const int sv = sv0 + q * per_cell;
    const int sx = sv % nsub, sy = (sv / nsub) % nsub, sz = sv / (nsub * nsub);
    wx[q] = x0 + ((sx + 0.5) * inv) * dx;
    wy[q] = y0 + ((sy + 0.5) * inv) * dy;
    wz[q] = z0 + ((sz + 0.5) * inv) * dz;
  }
  int best[N], own[N];
#pragma unroll
  for (int q = 0; q < N; ++q) { best[q] = INT32_MIN; own[q] = -1; }
  for (int p = 0; p < a.nprim; ++p) {
    const fdtd_voxel_prim* r = a.table + p;                       // wave-uniform
    if (r->role != FDTD_VOXEL_MATERIAL) continue;
    const int b0 = r->cbox[0], b1 = r->cbox[1], b2 = r->cbox[2], b3 = r->cbox[3], b4 = r->cbox[4], b5 = r->cbox[5];
    if (b3 < b0 || b4 < b1 || b5 < b2) continue;                  // holds no cell centre: invisible, as to the staircase
    const int l0 = max(b0 - 1, 0), l1 = max(b1 - 1, 0), l2 = max(b2 - 1, 0);
    const int h0 = min(b3 + 1, cx - 1), h1 = min(b4 + 1, cy - 1), h2 = min(b5 + 1, cz - 1);
    const bool gc = i >= l0 && i <= h0 && j >= l1 && j <= h1 && k >= l2 && k <= h2;
    if (__ballot(gc) == 0ull) continue;
    const unsigned gate = gc ? ((1u << N) - 1u) : 0u;
    const unsigned in = vx_test<N, true>(r, r->type, false, r->norm_dir, r->vert0, r->nvert, r->has_matrix != 0, a.verts, a.tol, wx, wy, wz, gate);
    const int prio = r->priority;
#pragma unroll
    for (int q = 0; q < N; ++q) {
      const bool win = ((in >> q) & 1u) && prio >= best[q];        // records in order: >= lets the later one win a tie
      best[q] = win ? prio : best[q];
      own[q] = win ? p : own[q];
    }
  }
  int pid[N];
#pragma unroll
  for (int q = 0; q < N; ++q) pid[q] = own[q] >= 0 ? a.table[own[q]].prop : a.nprop;
  if constexpr (FILL) {
    if (valid) {
#pragma unroll
      for (int q = 0; q < N; ++q) a.out[(size_t)w * (size_t)pts + (size_t)(sv0 + q * per_cell)] = (uint16_t)pid[q];
    }
  } else {
    bool same = true;
#pragma unroll
    for (int q = 1; q < N; ++q) same = same && pid[q] == pid[0];
    const int first = __shfl(pid[0], g * per_cell);
    const unsigned long long m = __ballot(!same || pid[0] != first);
    const unsigned long long gm = per_cell == 64 ? ~0ull : (((1ull << per_cell) - 1ull) << (g * per_cell));
    if (valid && sv0 == 0) a.out[cell] = (m & gm) ? SUB_MIXED : (uint16_t)first;
  }
}

struct SubEdgeArgs {
  int nx, ny, nz;
  const double* lines;
  int nsub;
  const double* prop_eps;            // [nprop + 1][3]
  const double* prop_kap;
  const uint8_t* prop_plain;
  long long ncand;
  const uint8_t* comp;               // per candidate edge: its component,
  const long long* idx;              // the flat index of its node (interior along a1 and a2, below the last along c: host),
  const int32_t* quarter;            // [ncand][4], (h1, h2) = (0,0) (0,1) (1,0) (1,1): the lattice slot of that cell, or -(material + 1)
  const uint16_t* lat;
  uint8_t* status;                   // bit 0: one of the four cells is mixed for the component; bit 1: some sample's material is not plain
  double* eps;
  double* kap;
};

__global__ __launch_bounds__(VX_BLOCK) void k_sub_edges(const SubEdgeArgs a) {
  const long long e = (long long)blockIdx.x * VX_BLOCK + threadIdx.x;
  if (e >= a.ncand) return;
  const int c = a.comp[e], a1 = (c + 1) % 3, a2 = (c + 2) % 3;
  const long long g = a.idx[e];
  const int n[3] = {(int)(g % a.nx), (int)((g / a.nx) % a.ny), (int)(g / ((long long)a.nx * a.ny))};
  const int off[3] = {0, a.nx, a.nx + a.ny};
  const int nsub = a.nsub, h = nsub / 2, pts = nsub * nsub * nsub;
  const int st[3] = {1, nsub, nsub * nsub};
  const double* L1 = a.lines + off[a1];
  const double* L2 = a.lines + off[a2];
  const double dn = (double)nsub;
  double ne = 0.0, nk = 0.0, den = 0.0;
  bool mixed = false, bad = false;
  for (int h1 = 0; h1 < 2; ++h1) {
    for (int h2 = 0; h2 < 2; ++h2) {
      const int q1 = n[a1] - 1 + h1, q2 = n[a2] - 1 + h2;            // 0 <= q <= n - 2: the node is interior along a1 and a2
      const double w = (L1[q1 + 1] - L1[q1]) * (L2[q2 + 1] - L2[q2]);
      const int code = a.quarter[4 * e + 2 * h1 + h2];
      const uint16_t* lat = code >= 0 ? a.lat + (size_t)code * (size_t)pts : nullptr;
      if (lat) {                                                     // the whole cell, not only the quarter: mixed for component c?
        const int p0 = (int)lat[0];
        const double e0 = a.prop_eps[3 * p0 + c], k0 = a.prop_kap[3 * p0 + c];
        for (int s = 1; s < pts; ++s) {
          const int pid = (int)lat[s];
          mixed = mixed || a.prop_eps[3 * pid + c] != e0 || a.prop_kap[3 * pid + c] != k0;
        }
      }
      for (int u1 = 0; u1 < h; ++u1) {
        for (int u2 = 0; u2 < h; ++u2) {
          const int s1 = h1 ? u1 : h + u1, s2 = h2 ? u2 : h + u2;
          const int base = s1 * st[a1] + s2 * st[a2];
          double R = 0.0, K = 0.0;
          for (int sc = 0; sc < nsub; ++sc) {
            const int pid = lat ? (int)lat[base + sc * st[c]] : -code - 1;
            const double ev = a.prop_eps[3 * pid + c], kv = a.prop_kap[3 * pid + c];
            bad = bad || a.prop_plain[pid] == 0;
            R = R + 1.0 / ev;
            K = K + kv;
          }
          ne = ne + (dn / R) * w;
          nk = nk + (K / dn) * w;
          den = den + w;
        }
      }
    }
  }
  a.status[e] = (uint8_t)((mixed ? 1 : 0) | (bad ? 2 : 0));
  a.eps[e] = ne / den;
  a.kap[e] = nk / den;
}

template <bool FILL>
void sub_launch_cells(const SubArgs& a) {
  const int nsub = a.nsub;
  const long long cpw = nsub == 2 ? 8 : 1;
  const long long waves = (a.ncells + cpw - 1) / cpw;
  const dim3 grid((unsigned)((waves + VX_BLOCK / 64 - 1) / (VX_BLOCK / 64))), block(VX_BLOCK);
  if (nsub == 8) hipLaunchKernelGGL((k_sub_cells<8, FILL>), grid, block, 0, 0, a);
  else hipLaunchKernelGGL((k_sub_cells<1, FILL>), grid, block, 0, 0, a);
}
}  // namespace

extern "C" int fdtd_voxel_subcell(int device, int nx, int ny, int nz, const double* lines, int nprim, const void* table, int nvert,
                                  const double* verts, double tol, const int32_t* rec_map, int nsub, int nprop, const double* prop_eps,
                                  const double* prop_kap, const uint8_t* prop_plain, const uint8_t* skip, int64_t cap, int8_t* comp,
                                  int64_t* idx, double* eps_rel, double* kap_e, int64_t* nlisted, int64_t* dropped) {
  if (!lines || (nvert > 0 && !verts) || !(tol >= 0.0) || (nsub != 2 && nsub != 4 && nsub != 8) || nprop < 0 || nprop >= (int)SUB_MIXED ||
      !prop_eps || !prop_kap || !prop_plain || !skip || cap < 0 || (cap > 0 && (!comp || !idx || !eps_rel || !kap_e)) || !nlisted)
    return fdtd_fail(nullptr, FDTD_E_ARG, "bad subcell argument");
  for (int p = 0; p <= nprop; ++p)
    for (int c = 0; c < 3; ++c)
      if (!(prop_eps[3 * p + c] > 0.0) || !(prop_kap[3 * p + c] >= 0.0) || !(prop_eps[3 * p + c] <= 1.7e308) || !(prop_kap[3 * p + c] <= 1.7e308))
        return fdtd_fail(nullptr, FDTD_E_ARG, "subcell: material %d needs finite eps > 0 and kappa >= 0 on every axis", p);
  int rc = FDTD_OK;
  *nlisted = 0;
  if (dropped) dropped[0] = dropped[1] = 0;
  try {
    std::vector<fdtd_voxel_prim> tab((size_t)(nprim > 0 ? nprim : 0));
    rc = vx_check_table(nx, ny, nz, nprim, table, nvert, tab.data());
    if (rc != FDTD_OK) return rc;
    if (nx < 3 || ny < 3 || nz < 3) return FDTD_OK;               // no interior node: every edge is dead
    bool any = false;
    for (int p = 0; p < nprim; ++p) {
      if (rec_map && rec_map[p] != 0) return fdtd_fail(nullptr, FDTD_E_ARG, "subcell: record %d delimits a voxel map: not supported", p);
      if (tab[p].role != FDTD_VOXEL_MATERIAL) continue;
      if (tab[p].prop < 0 || tab[p].prop >= nprop) return fdtd_fail(nullptr, FDTD_E_ARG, "subcell: record %d has material %d of %d", p, tab[p].prop, nprop);
      any = any || (tab[p].cbox[3] >= tab[p].cbox[0] && tab[p].cbox[4] >= tab[p].cbox[1] && tab[p].cbox[5] >= tab[p].cbox[2]);
    }
    if (!any) return FDTD_OK;                                     // no material holds a cell centre: no device work
    const long long cx = nx - 1, cy = ny - 1, cz = nz - 1, ncell = cx * cy * cz, nn = (long long)nx * ny * nz;
    if (ncell > (long long)INT32_MAX) return fdtd_fail(nullptr, FDTD_E_ARG, "subcell: more than 2^31 - 1 cells");
    const int pts = nsub * nsub * nsub;
    HIPCK(nullptr, hipSetDevice(device));
    double *d_lines = nullptr, *d_verts = nullptr, *d_peps = nullptr, *d_pkap = nullptr, *d_eps = nullptr, *d_kap = nullptr;
    fdtd_voxel_prim* d_tab = nullptr;
    uint16_t *d_code = nullptr, *d_lat = nullptr;
    int32_t *d_cells = nullptr, *d_quarter = nullptr;
    uint8_t *d_plain = nullptr, *d_comp = nullptr, *d_status = nullptr;
    long long* d_idx = nullptr;
    const size_t nl = (size_t)nx + (size_t)ny + (size_t)nz;
    std::vector<uint16_t> code((size_t)ncell);
    std::vector<int32_t> mixed_cells, quarter;
    std::vector<uint8_t> ccomp, status;
    std::vector<long long> cidx;
    std::vector<double> ceps, ckap;
#define VX(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess && rc == FDTD_OK) rc = fdtd_fail(nullptr, e_ == hipErrorOutOfMemory ? FDTD_E_NOMEM : FDTD_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); } while (0)
    VX(hipMalloc(&d_lines, nl * sizeof(double)));
    VX(hipMalloc(&d_verts, (size_t)(nvert > 0 ? nvert : 1) * sizeof(double)));
    VX(hipMalloc(&d_tab, (size_t)nprim * sizeof(fdtd_voxel_prim)));
    VX(hipMalloc(&d_code, (size_t)ncell * sizeof(uint16_t)));
    if (rc == FDTD_OK) {
      VX(hipMemcpy(d_lines, lines, nl * sizeof(double), hipMemcpyHostToDevice));
      if (nvert > 0) VX(hipMemcpy(d_verts, verts, (size_t)nvert * sizeof(double), hipMemcpyHostToDevice));
      VX(hipMemcpy(d_tab, tab.data(), (size_t)nprim * sizeof(fdtd_voxel_prim), hipMemcpyHostToDevice));
    }
    SubArgs a{nx, ny, nz, d_lines, nprim, d_tab, d_verts, tol, nsub, nprop, ncell, nullptr, d_code};
    if (rc == FDTD_OK) {
      sub_launch_cells<false>(a);
      VX(hipGetLastError());
      VX(hipDeviceSynchronize());
      if (rc == FDTD_OK) VX(hipMemcpy(code.data(), d_code, (size_t)ncell * sizeof(uint16_t), hipMemcpyDeviceToHost));
    }
    if (rc == FDTD_OK) {
      // the mixed cells, numbered in cell order (a cell's lattice slot is its position in that list)
      for (long long q = 0; q < ncell; ++q)
        if (code[(size_t)q] == SUB_MIXED) mixed_cells.push_back((int32_t)q);
        else if ((int)code[(size_t)q] > nprop) rc = fdtd_fail(nullptr, FDTD_E_DEVICE, "subcell: cell %lld came back with material %d", q, (int)code[(size_t)q]);
      // The candidate edges: the four edges per component around every mixed cell that have their four cells (interior along a1 and
      // a2), as keys component * nn + flat node index; sorted and made unique, they stand in list order.  The walk is over the mixed
      // cells, a surface, not over the grid's edges.
      const int lim[3] = {nx, ny, nz};
      std::vector<long long> keys;
      keys.reserve(rc == FDTD_OK ? mixed_cells.size() * 12 : 0);
      for (size_t m = 0; m < mixed_cells.size() && rc == FDTD_OK; ++m) {
        const long long cell = mixed_cells[m];
        const int q[3] = {(int)(cell % cx), (int)((cell / cx) % cy), (int)(cell / (cx * cy))};
        for (int c = 0; c < 3; ++c) {
          const int a1 = (c + 1) % 3, a2 = (c + 2) % 3;
          for (int o1 = 0; o1 < 2; ++o1)
            for (int o2 = 0; o2 < 2; ++o2) {
              int n[3];
              n[c] = q[c]; n[a1] = q[a1] + o1; n[a2] = q[a2] + o2;           // n[c] <= lim[c] - 2: a cell index
              if (n[a1] < 1 || n[a1] > lim[a1] - 2 || n[a2] < 1 || n[a2] > lim[a2] - 2) continue;   // an outer plane: no four cells
              keys.push_back((long long)c * nn + ((long long)n[2] * ny + n[1]) * nx + n[0]);
            }
        }
      }
      std::sort(keys.begin(), keys.end());
      keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
      for (size_t e = 0; e < keys.size() && rc == FDTD_OK; ++e) {
        const int c = (int)(keys[e] / nn), a1 = (c + 1) % 3, a2 = (c + 2) % 3;
        const long long g = keys[e] % nn;
        if (skip[(size_t)keys[e]] == 1) continue;
        const int n[3] = {(int)(g % nx), (int)((g / nx) % ny), (int)(g / ((long long)nx * ny))};
        int32_t q4[4];
        for (int h1 = 0; h1 < 2; ++h1)
          for (int h2 = 0; h2 < 2; ++h2) {
            int q[3];
            q[c] = n[c]; q[a1] = n[a1] - 1 + h1; q[a2] = n[a2] - 1 + h2;     // 0 <= q <= lim - 2 on every axis
            const long long cell = ((long long)q[2] * cy + q[1]) * cx + q[0];
            if (code[(size_t)cell] == SUB_MIXED)
              q4[2 * h1 + h2] = (int32_t)(std::lower_bound(mixed_cells.begin(), mixed_cells.end(), (int32_t)cell) - mixed_cells.begin());
            else
              q4[2 * h1 + h2] = -(int32_t)code[(size_t)cell] - 1;
          }
        ccomp.push_back((uint8_t)c); cidx.push_back(g);
        quarter.insert(quarter.end(), q4, q4 + 4);
      }
    }
    const size_t nmixed = mixed_cells.size(), ncand = cidx.size();
    if (rc == FDTD_OK && ncand > 0) {
      status.resize(ncand); ceps.resize(ncand); ckap.resize(ncand);
      VX(hipMalloc(&d_cells, nmixed * sizeof(int32_t)));
      VX(hipMalloc(&d_lat, nmixed * (size_t)pts * sizeof(uint16_t)));
      VX(hipMalloc(&d_peps, (size_t)(nprop + 1) * 3 * sizeof(double)));
      VX(hipMalloc(&d_pkap, (size_t)(nprop + 1) * 3 * sizeof(double)));
      VX(hipMalloc(&d_plain, (size_t)(nprop + 1)));
      VX(hipMalloc(&d_comp, ncand));
      VX(hipMalloc(&d_idx, ncand * sizeof(long long)));
      VX(hipMalloc(&d_quarter, ncand * 4 * sizeof(int32_t)));
      VX(hipMalloc(&d_status, ncand));
      VX(hipMalloc(&d_eps, ncand * sizeof(double)));
      VX(hipMalloc(&d_kap, ncand * sizeof(double)));
      if (rc == FDTD_OK) {
        VX(hipMemcpy(d_cells, mixed_cells.data(), nmixed * sizeof(int32_t), hipMemcpyHostToDevice));
        VX(hipMemcpy(d_peps, prop_eps, (size_t)(nprop + 1) * 3 * sizeof(double), hipMemcpyHostToDevice));
        VX(hipMemcpy(d_pkap, prop_kap, (size_t)(nprop + 1) * 3 * sizeof(double), hipMemcpyHostToDevice));
        VX(hipMemcpy(d_plain, prop_plain, (size_t)(nprop + 1), hipMemcpyHostToDevice));
        VX(hipMemcpy(d_comp, ccomp.data(), ncand, hipMemcpyHostToDevice));
        VX(hipMemcpy(d_idx, cidx.data(), ncand * sizeof(long long), hipMemcpyHostToDevice));
        VX(hipMemcpy(d_quarter, quarter.data(), ncand * 4 * sizeof(int32_t), hipMemcpyHostToDevice));
      }
      if (rc == FDTD_OK) {
        SubArgs f = a;
        f.ncells = (long long)nmixed; f.cells = d_cells; f.out = d_lat;
        sub_launch_cells<true>(f);
        VX(hipGetLastError());
        SubEdgeArgs b{nx, ny, nz, d_lines, nsub, d_peps, d_pkap, d_plain, (long long)ncand, d_comp, d_idx, d_quarter, d_lat, d_status, d_eps, d_kap};
        hipLaunchKernelGGL(k_sub_edges, dim3((unsigned)((ncand + VX_BLOCK - 1) / VX_BLOCK)), dim3(VX_BLOCK), 0, 0, b);
        VX(hipGetLastError());
        VX(hipDeviceSynchronize());
        if (rc == FDTD_OK) VX(hipMemcpy(status.data(), d_status, ncand, hipMemcpyDeviceToHost));
        if (rc == FDTD_OK) VX(hipMemcpy(ceps.data(), d_eps, ncand * sizeof(double), hipMemcpyDeviceToHost));
        if (rc == FDTD_OK) VX(hipMemcpy(ckap.data(), d_kap, ncand * sizeof(double), hipMemcpyDeviceToHost));
      }
    }
#undef VX
    hipFree(d_lines); hipFree(d_verts); hipFree(d_tab); hipFree(d_code); hipFree(d_lat); hipFree(d_cells); hipFree(d_quarter);
    hipFree(d_peps); hipFree(d_pkap); hipFree(d_plain); hipFree(d_comp); hipFree(d_idx); hipFree(d_status); hipFree(d_eps); hipFree(d_kap);
    if (rc != FDTD_OK) return rc;
    int64_t n = 0, drop[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {                         // count, then store if the list fits
      if (pass == 1 && n > cap) break;
      int64_t at = 0;
      for (size_t e = 0; e < ncand; ++e) {
        if (!(status[e] & 1)) continue;
        const uint8_t sk = skip[(size_t)ccomp[e] * (size_t)nn + (size_t)cidx[e]];
        if (sk == 2) { if (pass == 0) ++drop[0]; continue; }
        if (sk != 0) continue;
        if (status[e] & 2) { if (pass == 0) ++drop[1]; continue; }
        if (pass == 0) { ++n; continue; }
        comp[at] = (int8_t)ccomp[e]; idx[at] = (int64_t)cidx[e]; eps_rel[at] = ceps[e]; kap_e[at] = ckap[e];
        ++at;
      }
    }
    *nlisted = n;
    if (dropped) { dropped[0] = drop[0]; dropped[1] = drop[1]; }
    return FDTD_OK;
  } catch (...) {
    return fdtd_fail(nullptr, FDTD_E_NOMEM, "subcell: no host memory");
  }
}
