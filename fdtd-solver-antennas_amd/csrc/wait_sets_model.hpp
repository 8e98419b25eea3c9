// Host proof of wait_sets.hpp: for ONE tiling, every thread of every block enumerated, the blocks it depends on by the stencil (stated
// here cell by cell, with plain divisions, nothing shared with wait_sets.hpp but the geometry struct) must be in the set its block polls.
// Used by wait_sets_shim.cpp (tests/test_wait_sets_cpu.py drives the sweep) and by tools/wait_sets_check.cpp (the same sweep under
// the sanitizers).  Host only.
//
// The model.
//   H thread (k, j, c) — c = its four-cell group in the row — reads V of its own cells, of cell 4c + 4 (group c + 1), of row j + 1 and
//   of plane k + 1 (kernels.hip body_H: vz_ip / vy_ip, vz_jp / vx_jp, vy_kp / vx_kp), written by the E threads of those cells; and it
//   overwrites I values that E threads (k, j, c), (k, j, c + 1), (k, j + 1, c), (k + 1, j, c) read (body_E: iz_im / iy_im, iz_jm / ix_jm,
//   iy_km / ix_km): RAW and WAR are the same four threads.
//   E thread (k, j, c) of a later timestep of a launch mirrors it: H threads (k, j, c), (k, j, c - 1), (k, j - 1, c), (k - 1, j, c).
//   Mur candidates (kernels.hip mur_load_V reads them, mur_post_inline in body_E writes them): the candidate of a face point is written by
//   the E thread that owns the point's INNER node — same plane and row with group (inner cell) / 4 for an x face, row `in` for a y
//   face, plane `in` for a z face (in = b + 1 at a lower face, b - 1 at an upper one) — and is read by H thread (k, j, c) in place of:
//     vx        z face at k: (in_z(k), j, c), else y face at j: (k, in_y(j), c)          vy   z face at k: (in_z(k), j, c)
//     vz        y face at j: (k, in_y(j), c)                                             vz_jp  y face at j + 1: (k, in_y(j + 1), c)
//     vx_jp     z face at k: (in_z(k), j + 1, c), else y face at j + 1: (k, in_y(j + 1), c)
//     vy_kp     z face at k + 1: (in_z(k + 1), j, c)
//     vx_kp     z face at k + 1: (in_z(k + 1), j, c), else y face at j: (k + 1, in_y(j), c)
//     vz_ip     y face at j and cell 4c + 4 inside the grid: (k, in_y(j), c + 1); upper x face at cell 4c + 4: its own thread
//     vy_ip     z face at k and cell 4c + 4 inside the grid: (in_z(k), j, c + 1); upper x face at cell 4c + 4: its own thread
//     the four x-face candidates of a thread with a cell on an x face: (k, j, cx), (k, j + 1, cx), (k + 1, j, cx), cx = (inner cell) / 4
//   (rows and planes beyond the grid are not loaded as candidates).
#pragma once
#include <algorithm>
#include <vector>

#include "wait_sets.hpp"

enum WsWhat { WS_OK = 0, WS_FWD_MISSING = 1, WS_BACK_MISSING = 2, WS_MUR_CANDIDATE_MISSING = 3, WS_MUR_PLAIN_MISSING = 4, WS_LANES = 5,
              WS_FLAG_OUT_OF_TABLE = 6, WS_DECODE = 7 };
struct WsFail { int what, k, strip, pb, thread; long long flag; };   // the first failure of a tiling; flag: the one missing / wrong

inline WsGeom ws_make_geom(const int P4, const int ny, const int tys, const int nk, const int* b /* 6, or null */) {
  WsGeom g{};
  ws_set_P4(g, P4);
  g.ny = ny; g.tys = tys; g.nk = nk;
  g.nstrips = (ny + tys - 1) / tys;
  g.nbs = (std::min(tys, ny) * P4 + FDTD_BLOCK - 1) / FDTD_BLOCK;
  for (int f = 0; f < 6; ++f) g.b[f] = b ? b[f] : -1;
  return g;
}

class WsModel {
 public:
  explicit WsModel(const WsGeom& g) : g_(g), row_strip_(g.ny), row_base_(g.ny), stamp_((size_t)g.nk * g.nstrips * g.nbs, 0u) {
    for (int j = 0; j < g.ny; ++j) { row_strip_[j] = j / g.tys; row_base_[j] = (j % g.tys) * g.P4; }
  }
  // kind 0: wf_wait_flag against the H stencil, 1: wf_wait_back_flag against the E stencil
  WsFail check_plain(const int kind) {
    const int hop = 1 + g_.P4 / FDTD_BLOCK;
    if (2 * hop + 3 > 64) return WsFail{WS_LANES, -1, -1, -1, 2 * hop + 3, -1};
    for (int k = 0; k < g_.nk; ++k)
      for (int strip = 0; strip < g_.nstrips; ++strip)
        for (int pb = 0; pb * FDTD_BLOCK < threads_of(strip); ++pb) {
          begin_block();
          for (int lane = 0; lane < 64; ++lane) {
            const long long f = kind ? wf_wait_back_flag(g_, k, strip, pb, lane) : wf_wait_flag(g_, k, strip, pb, lane);
            if (f < 0) continue;
            if (lane >= 2 * hop + 3) return WsFail{WS_LANES, k, strip, pb, lane, f};
            if (!take(f)) return WsFail{WS_FLAG_OUT_OF_TABLE, k, strip, pb, lane, f};
          }
          const int lo = pb * FDTD_BLOCK, hi = std::min(lo + FDTD_BLOCK, threads_of(strip));
          for (int t = lo; t < hi; ++t) {
            const int j = strip * g_.tys + t / g_.P4, c = t % g_.P4;
            int dj = -1, di0 = -1;
            if (!ws_decode_thread(g_, strip, pb, t - lo, dj, di0) || dj != j || di0 != 4 * c) return WsFail{WS_DECODE, k, strip, pb, t - lo, -1};
            const int s = kind ? -1 : 1;
            long long need[4] = {flag_of(k, j, c), -1, -1, -1};
            if (c + s >= 0 && c + s < g_.P4) need[1] = flag_of(k, j, c + s);
            if (j + s >= 0 && j + s < g_.ny) need[2] = flag_of(k, j + s, c);
            if (k + s >= 0 && k + s < g_.nk) need[3] = flag_of(k + s, j, c);
            for (const long long f : need)
              if (f >= 0 && !has(f)) return WsFail{kind ? WS_BACK_MISSING : WS_FWD_MISSING, k, strip, pb, t - lo, f};
          }
          if (ws_decode_thread_beyond(strip, pb, hi - lo)) return WsFail{WS_DECODE, k, strip, pb, hi - lo, -1};
        }
    return WsFail{WS_OK, 0, 0, 0, 0, -1};
  }
  // wf_mur_wide + the set it selects, against the H stencil and the candidates (the geometry's faces b).  what = WS_LANES with k = -1: the
  // tiling is not one the host runs Mur faces on inside the launch (9 nbs flags do not fit the workgroup)
  WsFail check_mur() {
    if (9 * g_.nbs > FDTD_BLOCK) return WsFail{WS_LANES, -1, -1, -1, 9 * g_.nbs, -1};
    const int* b = g_.b;
    for (int k = 0; k < g_.nk; ++k)
      for (int strip = 0; strip < g_.nstrips; ++strip)
        for (int pb = 0; pb * FDTD_BLOCK < threads_of(strip); ++pb) {
          begin_block();
          const bool wide = wf_mur_wide(g_, k, strip, pb);
          for (int t = 0; t < (wide ? FDTD_BLOCK : 64); ++t) {
            const long long f = wide ? wf_wait_mur_flag(g_, k, strip, t) : wf_wait_flag(g_, k, strip, pb, t);
            if (f < 0) continue;
            if (wide && t >= 9 * g_.nbs) return WsFail{WS_LANES, k, strip, pb, t, f};
            if (!take(f)) return WsFail{WS_FLAG_OUT_OF_TABLE, k, strip, pb, t, f};
          }
          const bool kp = k + 1 < g_.nk;
          const bool z = k == b[4] || k == b[5], z1 = kp && (k + 1 == b[4] || k + 1 == b[5]);
          const int inz = k == b[4] ? k + 1 : k - 1, inz1 = k + 1 == b[4] ? k + 2 : k;
          const int lo = pb * FDTD_BLOCK, hi = std::min(lo + FDTD_BLOCK, threads_of(strip));
          int j = strip * g_.tys + lo / g_.P4, c = lo % g_.P4;
          for (int t = lo; t < hi; ++t, ++c) {
            if (c == g_.P4) { c = 0; ++j; }
            const bool jp = j + 1 < g_.ny;
            long long plain[4] = {flag_of(k, j, c), c + 1 < g_.P4 ? flag_of(k, j, c + 1) : -1, jp ? flag_of(k, j + 1, c) : -1, kp ? flag_of(k + 1, j, c) : -1};
            for (const long long f : plain)
              if (f >= 0 && !has(f)) return WsFail{WS_MUR_PLAIN_MISSING, k, strip, pb, t - lo, f};
            const bool y = j == b[2] || j == b[3], y1 = jp && (j + 1 == b[2] || j + 1 == b[3]);
            const int i0 = 4 * c;
            const bool xlo = b[0] == 0 && i0 == 0, xhi = b[1] >= 0 && b[1] - i0 >= 0 && b[1] - i0 < 4, xh_ip = b[1] >= 0 && i0 + 4 == b[1];
            if (!(z || z1 || y || y1 || xlo || xhi || xh_ip)) continue;
            const int iny = j == b[2] ? j + 1 : j - 1, iny1 = j + 1 == b[2] ? j + 2 : j;
            const bool in = i0 + 4 <= b1_or_last();   // cell 4c + 4 inside the grid (nx - 1 = the upper x index when the face is on)
            long long w[16];
            int n = 0;
            if (z) { w[n++] = flag_of(inz, j, c); if (jp) w[n++] = flag_of(inz, j + 1, c); if (in_next(c, in)) w[n++] = flag_of(inz, j, c + 1); }
            if (y) { w[n++] = flag_of(k, iny, c); if (kp && !z1) w[n++] = flag_of(k + 1, iny, c); if (in_next(c, in)) w[n++] = flag_of(k, iny, c + 1); }
            if (y1) w[n++] = flag_of(k, iny1, c);
            if (z1) w[n++] = flag_of(inz1, j, c);
            if (xh_ip) w[n++] = flag_of(k, j, c);
            if (xlo || xhi) {
              const int cx = (xhi ? b[1] - 1 : 1) / 4;
              w[n++] = flag_of(k, j, cx);
              if (jp) w[n++] = flag_of(k, j + 1, cx);
              if (kp) w[n++] = flag_of(k + 1, j, cx);
            }
            for (int q = 0; q < n; ++q)
              if (!has(w[q])) return WsFail{WS_MUR_CANDIDATE_MISSING, k, strip, pb, t - lo, w[q]};
          }
        }
    return WsFail{WS_OK, 0, 0, 0, 0, -1};
  }
  int nx_last = -1;   // nx - 1 for check_mur (the upper x face may be off)

 private:
  int threads_of(const int strip) const { return std::min(g_.tys, g_.ny - strip * g_.tys) * g_.P4; }
  long long flag_of(const int k, const int j, const int c) const {
    return ((long long)k * g_.nstrips + row_strip_[j]) * g_.nbs + ((row_base_[j] + c) / FDTD_BLOCK);
  }
  int b1_or_last() const { return nx_last; }
  bool in_next(const int c, const bool in) const { return in && c + 1 < g_.P4; }
  void begin_block() { ++gen_; }
  // a word of the flag table (so somebody publishes it: every block index below nbs of every strip-plane is dispatched, and a block beyond
  // the threads of a short last strip publishes at once)?  then it joins the set of the current block
  bool take(const long long f) {
    if (f >= (long long)stamp_.size()) return false;
    stamp_[(size_t)f] = gen_;
    return true;
  }
  bool has(const long long f) const { return stamp_[(size_t)f] == gen_; }
  bool ws_decode_thread_beyond(const int strip, const int pb, const int thread) const {   // the first thread beyond the strip, if the block has one
    int j, i0;
    return thread < FDTD_BLOCK && ws_decode_thread(g_, strip, pb, thread, j, i0);
  }
  WsGeom g_;
  std::vector<int> row_strip_, row_base_;
  std::vector<unsigned> stamp_;
  unsigned gen_ = 0u;
};

// check_mur for all 64 subsets of the six faces of an nx x ny x nk grid (bit f = face f on, at index 0 / n - 1 of its axis); 0 = proven,
// -1 = no tiling for Mur faces inside the launch (9 nbs > 256), else the first failure (its subset in *faces)
inline int ws_sweep_mur_faces(const int nx, const int ny, const int tys, const int nk, int* faces, WsFail* fail) {
  const int dim[3] = {nx, ny, nk};
  for (int s = 0; s < 64; ++s) {
    int b[6];
    for (int f = 0; f < 6; ++f) b[f] = ((s >> f) & 1) ? ((f & 1) ? dim[f / 2] - 1 : 0) : -1;
    WsModel m(ws_make_geom((nx + 3) / 4, ny, tys, nk, b));
    m.nx_last = nx - 1;
    *fail = m.check_mur();
    *faces = s;
    if (fail->what == WS_LANES && fail->k < 0) return -1;
    if (fail->what != WS_OK) return fail->what;
  }
  return 0;
}
