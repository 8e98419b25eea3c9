// Which per-block flags a block of the one-launch schedule (kernels.hip: k_step) polls — the arithmetic alone, integers only,
// for the device (kernel_common.hpp: wf_wait, wf_wait_back, wf_wait_mur; kernels.hip: body_H) and for the host (wait_sets_shim.cpp,
// tools/wait_sets_check.cpp: the brute-force proof that every block a block depends on is in the set it polls).
// A strip-plane (k, strip) is min(tys, ny - strip * tys) rows of P4 threads, thread t of it owns cells 4 * (t % P4) .. + 3 of row
// strip * tys + t / P4; block pb holds threads [pb * 256, pb * 256 + 256); its flag is word (k * nstrips + strip) * nbs + pb.
#pragma once

#ifndef FDTD_BLOCK
#define FDTD_BLOCK 256
#endif
#if defined(__HIPCC__) || defined(__CUDACC__)
#define WS_FN __host__ __device__ __forceinline__
#else
#define WS_FN inline
#endif
// Negative control of the host proof (make waitsets_host DROP=n): WAIT_SETS_DROP = n removes ONE clause; host builds only
#ifndef WAIT_SETS_DROP
#define WAIT_SETS_DROP 0
#elif WAIT_SETS_DROP != 0 && (defined(__HIPCC__) || defined(__CUDACC__))
#error "WAIT_SETS_DROP is for the host proof only"
#endif
#define WS_KEEP(n) (WAIT_SETS_DROP != (n))

// The geometry.  The functions that need no Mur faces take any struct with these members (template parameter G): the device hands them its
// parameter block as it is — building a WsGeom from it moved the SGPR counts of three k_step variants by one or two.
struct WsGeom {
  int P4, ny, tys, nstrips, nbs, nk;
  struct { unsigned mul, shr, d; } fd_P4;   // t / P4 as multiply-high + shift (fdtd_ctx.h: FastDiv, make_fastdiv), valid for 0 <= t < 2^31
  int b[6];                  // Mur faces: boundary index per face (x lo, x hi, y lo, y hi, z lo, z hi), -1 = off
};

WS_FN int ws_min(const int a, const int b) { return a < b ? a : b; }
template <class G> WS_FN unsigned ws_div_P4(const G& g, const unsigned t) {
#ifdef __HIP_DEVICE_COMPILE__
  return g.fd_P4.d == 1u ? t : __umulhi(t, g.fd_P4.mul) >> g.fd_P4.shr;
#else
  return g.fd_P4.d == 1u ? t : (unsigned)(((unsigned long long)t * g.fd_P4.mul) >> 32) >> g.fd_P4.shr;
#endif
}
// host side: the divider of make_fastdiv
inline void ws_set_P4(WsGeom& g, const int P4) {
  g.P4 = P4; g.fd_P4.mul = 0u; g.fd_P4.shr = 0u; g.fd_P4.d = (unsigned)P4;
  if (P4 > 1) {
    unsigned l = 0;
    while ((1ull << l) < (unsigned)P4) ++l;
    const unsigned p = 31 + l;
    g.fd_P4.mul = (unsigned)(((1ull << p) + (unsigned)P4 - 1) / (unsigned)P4);
    g.fd_P4.shr = p - 32;
  }
}

// thread t of block pb of strip `strip` -> row j and first cell i0; false beyond the strip
template <class G> WS_FN bool ws_decode_thread(const G& g, const int strip, const int pb, const int thread, int& j, int& i0) {
  const int t = pb * FDTD_BLOCK + thread;
  const int rows = ws_min(g.tys, g.ny - strip * g.tys);
  if (t >= rows * g.P4) return false;
  const int jj = (int)ws_div_P4(g, (unsigned)t);
  j = strip * g.tys + jj;
  i0 = (t - jj * g.P4) * 4;
  return true;
}

// E block (k, strip, pb) of a LATER timestep of a multi-step launch: the H flags of the previous timestep it waits for, one per lane
// (lanes 0 .. 2 * hop + 2 of wave 0): the blocks of threads t - P4 - 1 .. t + 255 of the strip-plane (its own cells, the row below, the
// element left of a group) — running into the previous strip's last rows at a strip's start — and the same block of plane k - 1.
// The mirror image of wf_wait_flag.
template <class G> WS_FN long long wf_wait_back_flag(const G& g, const int k, const int strip, const int pb, const int lane) {
  const int hop = 1 + g.P4 / FDTD_BLOCK;
  const int first = pb * FDTD_BLOCK - g.P4 - 1;                 // first strip-linear thread whose data is read (may be negative)
  const int t = lane;
  const long long row = ((long long)k * g.nstrips + strip) * g.nbs;
  long long f = -1;
  if (t <= hop) {                                               // same strip-plane: this block and the ones before it
    if ((t == 0 || WS_KEEP(4)) && pb - t >= 0 && (pb - t + 1) * FDTD_BLOCK - 1 >= first) f = row + pb - t;
  } else if (t <= 2 * hop + 1) {                                // previous strip's last blocks (always a full strip)
    const int q = t - hop - 1, Tp = g.tys * g.P4, lastb = (Tp - 1) / FDTD_BLOCK;
    if (WS_KEEP(5) && first < 0 && strip > 0 && lastb - q >= 0 && ws_min((lastb - q + 1) * FDTD_BLOCK, Tp) - 1 >= Tp + first) f = row - g.nbs + lastb - q;
  } else if (t == 2 * hop + 2) {                                // plane below
    if (WS_KEEP(6) && k > 0) f = row - (long long)g.nstrips * g.nbs + pb;
  }
  return f;
}
// H block (k, strip, pb): the E flags it waits for — the blocks whose output it reads / whose input it overwrites.  Threads t .. t+255 of
// the strip-plane read rows j and j+1 (thread t + P4) and the element right of their group (thread t + 1): strip-linear
// threads [pb*256, pb*256 + 256 + P4] at plane k — running into the next strip's first rows at a strip's end — and the
// same block at plane k + 1.  One lane per flag.
template <class G> WS_FN long long wf_wait_flag(const G& g, const int k, const int strip, const int pb, const int lane) {
  const int hop = 1 + g.P4 / FDTD_BLOCK;
  const int rows = ws_min(g.tys, g.ny - strip * g.tys);
  const int T = rows * g.P4;                                   // threads of this strip-plane
  const int last = pb * FDTD_BLOCK + FDTD_BLOCK + g.P4;        // last strip-linear thread whose data is read
  const int t = lane;
  const long long row = ((long long)k * g.nstrips + strip) * g.nbs;
  long long f = -1;
  if (t <= hop) {                                              // same strip, this block and the ones behind it
    if ((t == 0 || WS_KEEP(1)) && (pb + t) * FDTD_BLOCK <= ws_min(last, T - 1)) f = row + pb + t;
  } else if (t <= 2 * hop + 1) {                               // next strip's first blocks
    const int q = t - hop - 1;
    if (WS_KEEP(2) && last >= T && strip + 1 < g.nstrips && q < g.nbs && q * FDTD_BLOCK <= last - T) f = row + g.nbs + q;
  } else if (t == 2 * hop + 2) {                               // plane above
    if (WS_KEEP(3) && k + 1 < g.nk) f = row + (long long)g.nstrips * g.nbs + pb;
  }
  return f;
}
// Mur faces inside the one-launch schedule, the WIDE set: every block of strips s - 1 .. s + 1 at planes k - 1 .. k + 1 (9 nbs flags, one
// thread each; the host takes this schedule only while they fit the workgroup)
template <class G> WS_FN long long wf_wait_mur_flag(const G& g, const int k, const int strip, const int thread) {
  const int t = thread, nbs = g.nbs;
  const int dk = t / (3 * nbs) - 1, r = t - (dk + 1) * 3 * nbs, ds = r / nbs - 1, q = r - (ds + 1) * nbs;
  const int kk = k + dk, ss = strip + ds;
  if (!WS_KEEP(12) && dk < 0) return -1;
  if (!WS_KEEP(13) && dk > 0) return -1;
  if (!WS_KEEP(14) && ds < 0) return -1;
  if (!WS_KEEP(15) && ds > 0) return -1;
  if (t < 9 * nbs && kk >= 0 && kk < g.nk && ss >= 0 && ss < g.nstrips) return ((long long)kk * g.nstrips + ss) * nbs + q;
  return -1;
}
// Does H block (k, strip, pb) of a grid with Mur faces take the wide set?  Away from the y and z faces the candidates a block loads were
// written by E blocks of the plain set — by the thread of the same cells (x faces; the row / plane in front of an upper face) —; a block
// that holds a row or a plane ON a y / z face (candidates from the row / plane behind it, or one further ahead than the plain set
// reaches), and every block of a grid whose upper x face starts a four-cell group (the inner node belongs to the thread before), does.
WS_FN bool wf_mur_wide(const WsGeom& g, const int k, const int strip, const int pb) {
  const int rows = ws_min(g.tys, g.ny - strip * g.tys);
  const int jlo = strip * g.tys + (int)ws_div_P4(g, (unsigned)(pb * FDTD_BLOCK));
  const int jhi = strip * g.tys + ws_min(rows - 1, (int)ws_div_P4(g, (unsigned)(pb * FDTD_BLOCK + FDTD_BLOCK - 1)));
  return (WS_KEEP(7) && k == g.b[4]) || (WS_KEEP(8) && k == g.b[5]) || (WS_KEEP(9) && g.b[2] >= jlo && g.b[2] <= jhi) ||
         (WS_KEEP(10) && g.b[3] >= jlo && g.b[3] <= jhi) || (WS_KEEP(11) && g.b[1] >= 0 && (g.b[1] & 3) == 0);
}
