// libfdtd_waitsets.so (make waitsets_host; g++, no GPU): the functions of wait_sets.hpp and the per-tiling brute force of
// wait_sets_model.hpp behind a C interface, for tests/test_wait_sets_cpu.py (ctypes).  Built with -DWAIT_SETS_DROP=n the library lacks one
// clause of the wait sets: the negative control of the proof.
#include "wait_sets_model.hpp"

extern "C" {
int ws_drop() { return WAIT_SETS_DROP; }
// geometry as the host lays it out: nstrips, nbs and the P4 divider follow from (P4, ny, tys, nk); b: six face indices (-1 = off) or null
void ws_geom(WsGeom* g, int P4, int ny, int tys, int nk, const int* b) { *g = ws_make_geom(P4, ny, tys, nk, b); }
long long ws_wait_flag(const WsGeom* g, int k, int strip, int pb, int lane) { return wf_wait_flag(*g, k, strip, pb, lane); }
long long ws_wait_back_flag(const WsGeom* g, int k, int strip, int pb, int lane) { return wf_wait_back_flag(*g, k, strip, pb, lane); }
long long ws_wait_mur_flag(const WsGeom* g, int k, int strip, int thread) { return wf_wait_mur_flag(*g, k, strip, thread); }
int ws_mur_wide(const WsGeom* g, int k, int strip, int pb) { return wf_mur_wide(*g, k, strip, pb) ? 1 : 0; }
int ws_decode(const WsGeom* g, int strip, int pb, int thread, int* j, int* i0) { return ws_decode_thread(*g, strip, pb, thread, *j, *i0) ? 1 : 0; }
// every (k, strip, pb, lane) of the geometry, in the layout of the device's dump (fdtd_debug_wait_sets): out[5][nk][nstrips][nbs][256] =
// wf_wait_flag, wf_wait_back_flag (lanes < 64, else -1), wf_wait_mur_flag, wf_mur_wide in every lane, the thread decode (j << 32 | i0, or -1)
void ws_dump(const WsGeom* g, long long* out) {
  const size_t n = (size_t)g->nk * g->nstrips * g->nbs * FDTD_BLOCK;
  size_t e = 0;
  for (int k = 0; k < g->nk; ++k)
    for (int strip = 0; strip < g->nstrips; ++strip)
      for (int pb = 0; pb < g->nbs; ++pb)
        for (int t = 0; t < FDTD_BLOCK; ++t, ++e) {
          out[e] = t < 64 ? wf_wait_flag(*g, k, strip, pb, t) : -1;
          out[n + e] = t < 64 ? wf_wait_back_flag(*g, k, strip, pb, t) : -1;
          out[2 * n + e] = wf_wait_mur_flag(*g, k, strip, t);
          out[3 * n + e] = wf_mur_wide(*g, k, strip, pb) ? 1 : 0;
          int j = 0, i0 = 0;
          out[4 * n + e] = ws_decode_thread(*g, strip, pb, t, j, i0) ? ((long long)j << 32) | (long long)i0 : -1;
        }
}
// The brute force of one tiling.  which: 0 = wf_wait_flag, 1 = wf_wait_back_flag, 2 = wf_mur_wide with the set it selects (faces g->b; nx_last = nx - 1).
// Returns WsFail::what (0 = proven) and leaves the first failure in *fail.
int ws_check(const WsGeom* g, int which, int nx_last, WsFail* fail) {
  WsModel m(*g);
  m.nx_last = nx_last;
  *fail = which == 2 ? m.check_mur() : m.check_plain(which);
  return fail->what;
}
// which = 2 for all 64 subsets of the six faces of an nx x ny x nk grid (bit f of the subset = face f on, at index 0 / n - 1 of its axis);
// stops at the first failure and leaves its subset in *faces.  Returns 0 = proven, -1 = not a tiling for Mur faces inside the launch.
int ws_check_mur_faces(int nx, int ny, int tys, int nk, int* faces, WsFail* fail) {
  return ws_sweep_mur_faces(nx, ny, tys, nk, faces, fail);
}
}
