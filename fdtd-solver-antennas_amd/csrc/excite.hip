// excite.hip — H-field excitations on listed faces (include/fdtd_hip_excite.h).
//
// The operator and the H kernels stay what they are; behind the H update a listed face current is replaced by (hard entry) or
// increased by (soft entries) amp * sigH[step - delay].  The lists are feeds — a frill, an annulus, a plane of a launcher: a few
// thousand faces at most — so k_excite is a latency floor like k_conformal and k_planewave: one thread per DISTINCT face, its record
// (offset, component and hard flag, its range of soft entries: 16 bytes, one load) read from consecutive memory by consecutive
// lanes, the pulse table (a few thousand floats, shared by all lanes) through L1, at most one scattered load and one scattered
// store of the current.  The host has grouped the entries by face, the soft ones in list order, so the fp32 order the header
// spells does not depend on the launch shape, and no face is written by two threads: no atomics.  Every statement is one fp32
// operation (-ffp-contract=off), so a host restatement on top of the oracle's half-steps reproduces it bit for bit.  No state.
#include "corrections.hpp"
#include "../../include/fdtd_hip_excite.h"

#include <algorithm>
#include <numeric>
#include <vector>

namespace {

struct ExciteArgs {
  float* I0; float* I1; float* I2;
  const int4* face;        // x: offset of the face's node, y: component | hard << 2, z: first soft entry, w: soft entries
  const float* hamp; const int* hdelay;   // [nface], read where the face has a hard entry
  const float* samp; const int* sdelay;   // [nsoft], grouped by face
  const float* sig;
  long long step;
  int nsig, n;
};

__global__ __launch_bounds__(256) void k_excite(const ExciteArgs a) {
  const int f = (int)(blockIdx.x * 256u + threadIdx.x);
  if (f >= a.n) return;
  const int4 fc = a.face[f];
  const int c = fc.y & 3;
  float* I = c == 0 ? a.I0 : c == 1 ? a.I1 : a.I2;
  const long o = fc.x;
  float v;
  if (fc.y & 4) {          // the hard entry first: it holds the face at zero outside the table
    const long long p = a.step - a.hdelay[f];
    const float s = (p >= 0 && p < (long long)a.nsig) ? a.sig[p] : 0.0f;
    v = a.hamp[f] * s;
  } else {
    v = I[o];
  }
  bool changed = (fc.y & 4) != 0;
  for (int q = fc.z; q < fc.z + fc.w; ++q) {
    const long long p = a.step - a.sdelay[q];
    if (p < 0 || p >= (long long)a.nsig) continue;   // outside the table: nothing is added, not even a zero
    const float t = a.samp[q] * a.sig[p];
    v = v + t;
    changed = true;
  }
  if (changed) I[o] = v;
}

void excite_free(fdtd_ctx* c) {
  fdtd_ctx::ExciteSet& x = c->excite;
  hipFree(x.face); hipFree(x.hamp); hipFree(x.hdelay); hipFree(x.samp); hipFree(x.sdelay); hipFree(x.sig);
  x = fdtd_ctx::ExciteSet{};
}

void launch_excite(fdtd_ctx* c, long long step, hipStream_t s) {
  const fdtd_ctx::ExciteSet& x = c->excite;
  if (x.n <= 0) return;
  ExciteArgs a{c->p.I[0], c->p.I[1], c->p.I[2], x.face, x.hamp, x.hdelay, x.samp, x.sdelay, x.sig, step, x.nsig, x.n};
  hipLaunchKernelGGL(k_excite, dim3((unsigned)((x.n + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace

#ifndef __HIP_DEVICE_COMPILE__   // (host data: corrections.hpp)
const CorrectionRow corr_excite = {
    "H-field excitations", /*no_links*/ true, /*volume*/ false,
    [](const fdtd_ctx* c) { return c->excite.n > 0; },
    nullptr, launch_excite, excite_free, nullptr, nullptr};
#endif

extern "C" {

int fdtd_excite_set(fdtd_ctx* c, int nhard, const int64_t* idxH, const int8_t* compH, const float* ampH, const int32_t* delayH,
                    int nsoft, const int64_t* idxS, const int8_t* compS, const float* ampS, const int32_t* delayS,
                    const float* sigH, int nsigH) {
  if (!c) return FDTD_E_ARG;
  if (nhard < 0 || nsoft < 0 || (nhard > 0 && (!idxH || !compH || !ampH || !delayH)) || (nsoft > 0 && (!idxS || !compS || !ampS || !delayS)) ||
      ((nhard > 0 || nsoft > 0) && (!sigH || nsigH < 1)))
    return fdtd_fail(c, FDTD_E_ARG, "fdtd_excite_set: bad argument");
  if (int r = correction_set_begin(c, corr_excite, "fdtd_excite_set", nhard > 0 || nsoft > 0)) return r;
  const int64_t nn[3] = {c->d.nx, c->d.ny, c->d.nz};
  // every entry: (key = 3 * index + component, local offset), checked
  const int ntot = nhard + nsoft;
  std::vector<int64_t> key((size_t)ntot);
  std::vector<int> off((size_t)ntot);
  for (int e = 0; e < ntot; ++e) {
    const bool hard = e < nhard;
    const int q = hard ? e : e - nhard;
    const char* what = hard ? "hard" : "soft";
    const int m = (hard ? compH : compS)[q];
    const int64_t g = (hard ? idxH : idxS)[q];
    int64_t pos[3];
    if (!sparse_decode(c, g, m, pos, &off[e])) return fdtd_fail(c, FDTD_E_ARG, "fdtd_excite_set: %s face %d out of range", what, q);
    // a face spans one cell along both transverse axes
    if (pos[(m + 1) % 3] >= nn[(m + 1) % 3] - 1 || pos[(m + 2) % 3] >= nn[(m + 2) % 3] - 1)
      return fdtd_fail(c, FDTD_E_ARG, "fdtd_excite_set: %s face %d does not exist", what, q);
    if ((hard ? delayH : delayS)[q] < 0) return fdtd_fail(c, FDTD_E_ARG, "fdtd_excite_set: %s face %d has a negative delay", what, q);
    key[e] = g * 3 + m;
  }
  {
    std::vector<int64_t> hk(key.begin(), key.begin() + nhard);
    if (sparse_doubles(hk)) return fdtd_fail(c, FDTD_E_ARG, "fdtd_excite_set: a face given twice in the hard list");
  }
  // group by face: entries sorted by (key, position in the lists) — a stable sort keeps a face's hard entry in front of its soft
  // entries and those in list order
  std::vector<int> order((size_t)ntot);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[a] < key[b]; });
  std::vector<int4> face;
  std::vector<float> hamp, samp;
  std::vector<int> hdelay, sdelay;
  for (int n = 0; n < ntot; ++n) {
    const int e = order[n];
    if (n == 0 || key[e] != key[order[n - 1]]) {
      face.push_back(make_int4(off[e], (int)(key[e] % 3), (int)samp.size(), 0));
      hamp.push_back(0.f); hdelay.push_back(0);
    }
    if (e < nhard) {
      face.back().y |= 4;
      hamp.back() = ampH[e]; hdelay.back() = delayH[e];
    } else {
      face.back().w++;
      samp.push_back(ampS[e - nhard]); sdelay.push_back(delayS[e - nhard]);
    }
  }
  if (int r = correction_set_replace(c, corr_excite)) return r;
  if (ntot == 0) return FDTD_OK;
  fdtd_ctx::ExciteSet& x = c->excite;
  hipError_t e = to_device(&x.face, face);
  if (e == hipSuccess) e = to_device(&x.hamp, hamp);
  if (e == hipSuccess) e = to_device(&x.hdelay, hdelay);
  if (e == hipSuccess) e = to_device(&x.samp, samp);
  if (e == hipSuccess) e = to_device(&x.sdelay, sdelay);
  if (e == hipSuccess) e = to_device(&x.sig, std::vector<float>(sigH, sigH + nsigH));
  if (e != hipSuccess) return correction_set_failed(c, corr_excite, "fdtd_excite_set", e);
  x.n = (int)face.size();
  x.nsig = nsigH;
  return FDTD_OK;
}

}  // extern "C"
