/* fdtd_hip_voxel.h — rasterise CSXCAD primitives (boxes, spheres, cylinders, shells, polygons, wires, triangle meshes) onto the Yee grid on the
 * device.  Exported by libfdtd_hip.so only; not part of fdtd_hip.h nor of FDTD_ABI_VERSION (as the other feature headers).
 *
 * The numpy rasteriser primitives.rasterise_spec is the specification; fdtd_voxelize gives the same owners bit for bit, because
 * both spell the arithmetic below in float64 with + - * and comparisons only, in exactly this association, and the library is
 * compiled with -ffp-contract=off.
 *
 * Table: nprim records of struct fdtd_voxel_prim in ownership order.  A material record (role 0) is tested on the cell centres
 * 0.5 * (l[i] + l[i + 1]) inside its inclusive index box cbox, a metal record (role 1) on the nodes inside nbox; a point outside
 * the index box is outside the primitive.  The owner of a cell is the record of the highest priority that holds its centre, the
 * later record on a tie.  The owner of an edge (component c at node n) is, by the same rule, among the metal records that hold
 * both n and n + e_c; -1: none.
 *
 * With t = +tol for a metal and -tol for a material, (x, y, z) the point in metres, par = p[0..7]:
 *   transform (has_matrix): x' = ((m[0] x + m[1] y) + m[2] z) + m[3], y' and z' with m[4..7], m[8..11]; then x, y, z = x', y', z'.
 *   BOX        p = lo[3], hi[3]:  x >= p0 - t && x <= p3 + t, likewise y (p1, p4) and z (p2, p5).
 *   SPHERE     p = c[3], r:       d = (x, y, z) - c; d2 = (dx dx + dy dy) + dz dz; re = r + t; re >= 0 && d2 <= re re.
 *   SPH. SHELL p = c[3], r, w:    ro = (r + 0.5 w) + t; ri = (r - 0.5 w) - t; ro >= 0 && d2 <= ro ro && (ri <= 0 || d2 >= ri ri).
 *   CYLINDER   p = a[3], b[3], r: d = b - a; L = (dx dx + dy dy) + dz dz; w = (x, y, z) - a; s = (wx dx + wy dy) + wz dz;
 *                                 ww = (wx wx + wy wy) + wz wz; q = ww L - s s; tt = (tol tol) L; e = s - L;
 *                                 axial, metal:    (s >= 0 || s s <= tt) && (e <= 0 || e e <= tt)
 *                                 axial, material: (s >= 0 && s s >= tt) && (e <= 0 && e e >= tt)
 *                                 re = r + t; axial && re >= 0 && q <= (re re) L.
 *   CYL. SHELL p = a[3], b[3], r, w: axial as above; ro, ri as for the spherical shell;
 *                                 ro >= 0 && q <= (ro ro) L && (ri <= 0 || q >= (ri ri) L).
 *   DISC       p = a[3], -, -, -, r (a cylinder with start == stop, normal to local z), metals only:
 *                                 d = (x, y, z) - a; re = r + t; dz <= tol && dz >= -tol && dx dx + dy dy <= re re.
 *   POLYGON    p = elevation; norm_dir n; vertices (u, v) = verts[vert0 + 2 e ...], metals only:
 *                                 pn, pu, pv = the coordinates n, (n + 1) % 3, (n + 2) % 3; dn = pn - p0; dn <= tol && dn >= -tol;
 *              in the plane, for every edge e from A = vertex e to B = vertex (e + 1) % nvert:
 *                                 du = Bu - Au; dv = Bv - Av; wu = pu - Au; wv = pv - Av;
 *                                 crossing: (Av > pv) != (Bv > pv) && (dv > 0 ? wu dv < wv du : wu dv > wv du)  -> parity ^= 1
 *                                 near: eu = pu - Bu; ev = pv - Bv; L = du du + dv dv; s = wu du + wv dv; ww = wu wu + wv wv;
 *                                       s <= 0 ? ww <= tol tol : s >= L ? eu eu + ev ev <= tol tol : ww L - s s <= (tol tol) L
 *                                 metal: parity || near (any edge);  material: parity && !near.
 *   LINPOLY    p = lo, hi along n: pn >= p0 - t && pn <= p1 + t, and the polygon's test in the plane.
 *   WIRE       p = r; points (x, y, z) = verts[vert0 + 3 e ...], metals only: re = r + t; re2 = re re; any segment e from A to B
 *              (one point: A = B):  d = B - A; w = p - A; g = p - B; L, s, ww as for the cylinder; gg = (gx gx + gy gy) + gz gz;
 *                                 s <= 0 ? ww <= re2 : s >= L ? gg <= re2 : ww L - s s <= re2 L.   (this is seg_near(w, g, d, re2))
 *   POLYHEDRON a CLOSED triangle mesh (every undirected edge used by an even number of triangles; facet normals and the order of a
 *              triangle's corners do not matter); nvert = 3 ntri points, the triangle's corners A, B, C = verts[vert0 + 9 tr ...]
 *              (x, y, z each); par unused.  A point is inside when the ray from it towards +x crosses an odd number of triangles.
 *              With g = 2 tol, per triangle:
 *                gate:  inyz = y >= min(Ay, By, Cy) - g && y <= max(...) + g && z >= min(Az, Bz, Cz) - g && z <= max(...) + g;
 *                       a triangle whose gate a point fails neither crosses its ray nor is near it.
 *                e1 = B - A; e2 = C - A; n = e1 x e2, each component a b - c d: nx = e1y e2z - e1z e2y, ny = e1z e2x - e1x e2z,
 *                nz = e1x e2y - e1y e2x; nn = (nx nx + ny ny) + nz nz; w = p - A; s = (nx wx + ny wy) + nz wz.
 *                projected hit: for each edge (A B, B C, C A) take its end points in CANONICAL order, a = the end with the smaller
 *                       z, the smaller y on a tie (so both triangles of a shared edge evaluate the identical expression, and a ray
 *                       through a shared edge or vertex is counted once):  du = by - ay; dv = bz - az; wu = y - ay; wv = z - az;
 *                       crossing: (az > z) != (bz > z) && wu dv < wv du;  in_proj = the parity of the three crossings.
 *                ray:   nx != 0 && inyz && in_proj && (nx > 0 ? s < 0 : s > 0)  -> parity ^= 1.
 *                near (only inside the box: inyz && x >= min(Ax, Bx, Cx) - g && x <= max(...) + g):
 *                       c_k = ((b - a) x (p - a)) . n >= 0 for the edges A->B, B->C, C->A in the triangle's own order, the cross
 *                       product as above (d = b - a, v = p - a: dy vz - dz vy, dz vx - dx vz, dx vy - dy vx), the dot product
 *                       (cx nx + cy ny) + cz nz;  all three: s s <= (tol tol) nn;  otherwise: seg_near(p - a, p - b, b - a, tol tol)
 *                       of any of the three edges.
 *              metal: parity || near (any triangle);  material: parity && !near.  A face exactly on a mesh plane is therefore
 *              decided by `near` for a metal (its nodes are held) and by the half-open crossing rule for a material's cell centres.
 *
 * Voxel maps (fdtd_voxelize_maps; discmaterial.lookup_spec is the same text in numpy): a material record p with rec_map[p] = m + 1 is a
 * delimiter of map m and holds a cell centre iff its own predicate above holds it AND the map holds it.  With M = maps[m].m and
 * (x, y, z) the centre in world metres (NOT the record's local frame):
 *   q_x = ((M[0] x + M[1] y) + M[2] z) + M[3], q_y with M[4..7], q_z with M[8..11];
 *   per axis a with the n_a lines L_a: i_a = (the number of t with L_a[t] <= q_a) - 1; the point has a voxel iff
 *   0 <= i_a <= n_a - 2 on all three axes (half-open: L[0] <= q < L[n - 1]; a NaN has none);
 *   voxel = (i_z (n_y - 1) + i_y) (n_x - 1) + i_x (in 64 bits), v = data[voxel];
 *   the map holds the point iff it has a voxel && (v != 0 || use_db_background).
 * Only comparisons follow the three q.  cell_voxel is `voxel` where the owning record has a map, -1 elsewhere.  Ownership is
 * unchanged: the highest priority, the later record on a tie — so index 0 is transparent (unless use_db_background) and shows
 * whatever lower priority lies under it.
 */
#ifndef FDTD_HIP_VOXEL_H
#define FDTD_HIP_VOXEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { FDTD_VOXEL_BOX = 0, FDTD_VOXEL_SPHERE, FDTD_VOXEL_SPHERICAL_SHELL, FDTD_VOXEL_CYLINDER, FDTD_VOXEL_CYLINDRICAL_SHELL,
       FDTD_VOXEL_DISC, FDTD_VOXEL_POLYGON, FDTD_VOXEL_LINPOLY, FDTD_VOXEL_WIRE, FDTD_VOXEL_POLYHEDRON,
       FDTD_VOXEL_NTYPES };
enum { FDTD_VOXEL_MATERIAL = 0, FDTD_VOXEL_METAL = 1 };

typedef struct fdtd_voxel_prim {
  int32_t type, role, prop, priority, order;   /* prop: index of the material / metal; order: drawing order (== record index) */
  int32_t vert0, nvert;                        /* offset into verts (in doubles) and number of vertices / points (3 per triangle) */
  int32_t norm_dir, has_matrix, pad;
  int32_t cbox[6], nbox[6];                    /* inclusive index boxes x0 y0 z0 x1 y1 z1 on the cell / node grid; x0 > x1: empty */
  double par[8];
  double m[12];                                /* 3x4 world -> local, metres */
} fdtd_voxel_prim;                             /* 248 bytes */

/* lines: the nx + ny + nz mesh lines in metres; table: nprim records; verts: nvert doubles.  cell_owner: int32 [nz-1][ny-1][nx-1],
 * edge_owner: int32 [3][nz][ny][nx], host pointers, either may be NULL (that pass is not run).  Returns FDTD_OK or a negative
 * FDTD_E_* code (message: fdtd_last_error(NULL)); index boxes are clipped to the grid, a record with an unknown type, vertices
 * outside verts or a polyhedron whose nvert is no multiple of 3 is FDTD_E_ARG.  nprim == 0 and primitives outside the grid give owners of -1. */
int fdtd_voxelize(int device, int nx, int ny, int nz, const double* lines, int nprim, const void* table, int nvert,
                  const double* verts, double tol, int32_t* cell_owner, int32_t* edge_owner);

/* One voxel map: m the 3 x 4 world (metres) -> map coordinates; lines[a] the n[a] >= 2 strictly increasing lines of axis a; data
 * uint8 [n[2]-1][n[1]-1][n[0]-1], x fastest, ndata = its length (checked against n); host pointers. */
typedef struct fdtd_voxel_map {
  double m[12];
  const double* lines[3];
  const uint8_t* data;
  int64_t ndata;
  int32_t n[3];
  int32_t use_db_background;
} fdtd_voxel_map;                              /* 152 bytes */

enum { FDTD_VOXEL_MAX_MAPS = 4 };

/* fdtd_voxelize with voxel maps: rec_map int32 [nprim] (0: none, m + 1: the record delimits maps[m]; NULL with nmaps == 0), maps
 * [nmaps <= FDTD_VOXEL_MAX_MAPS], cell_voxel int32 [nz-1][ny-1][nx-1] (needs cell_owner; NULL: not wanted).  The records without a map
 * are rasterised as fdtd_voxelize does; one further launch merges the mapped records into those owners by (priority, record index).
 * FDTD_E_ARG: a mapped record that is a metal or a polyhedron, rec_map out of range, a map with n < 2, lines that do not increase,
 * more than 2^31 - 1 voxels or ndata != (n[0]-1)(n[1]-1)(n[2]-1).  With nmaps == 0 the owners are fdtd_voxelize's and cell_voxel is -1. */
int fdtd_voxelize_maps(int device, int nx, int ny, int nz, const double* lines, int nprim, const void* table, int nvert,
                       const double* verts, double tol, int32_t* cell_owner, int32_t* edge_owner, const int32_t* rec_map, int nmaps,
                       const fdtd_voxel_map* maps, int32_t* cell_voxel);

#ifdef __cplusplus
}
#endif
#endif
