// host_tables.hpp — host-side table logic of libfdtd_hip.so without a single HIP call, so that it compiles with any host
// compiler and runs under its sanitizers (tests/host_tables_main.cpp).
//
//  * trim_active: which indices of a CPML axis carry a layer that DOES something.  The slot ranges an axis is handed
//    (fdtd_set_cpml) are storage ranges; some of their indices have identity coefficients (b = 0, c = 0, 1 / kappa = 1): there
//    psi <- 0 * psi + 0 * d = +-0 and d <- 1 * d + psi = d, i.e. the psi loads, the arithmetic and the psi stores change nothing.
//  * dedup_rows: the per-cell class bytes as one id per (k, j) row plus the table of distinct rows.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string_view>
#include <unordered_map>
#include <vector>

namespace host_tables {

// Active sub-ranges of the two end-anchored storage ranges [0, lo) and [hi, n) of one (axis, E / H side): [a0, a1) and [b0, b1), both
// possibly empty (then begin == end).
struct ActiveRanges {
  int a0, a1, b0, b1;
  int count() const { return (a1 - a0) + (b1 - b0); }
};

inline bool inert(float b, float c, float ik) { return b == 0.0f && c == 0.0f && ik == 1.0f; }   // (-0.0f == 0.0f)

// Trim one range [begin, end) from both ends while the index is inert; an inert index between two active ones stays.
inline void trim_range(const float* b, const float* c, const float* ik, int begin, int end, int* out_begin, int* out_end) {
  while (begin < end && inert(b[begin], c[begin], ik[begin])) ++begin;
  while (end > begin && inert(b[end - 1], c[end - 1], ik[end - 1])) --end;
  if (begin >= end) begin = end = 0;
  *out_begin = begin; *out_end = end;
}

// b, c, ik: the axis' coefficient tables, n entries each.  lo: end of the low storage range; hi: start of the high one (hi >= n: none).
inline ActiveRanges trim_active(const float* b, const float* c, const float* ik, int n, int lo, int hi) {
  ActiveRanges r{0, 0, 0, 0};
  if (lo > n) lo = n;
  trim_range(b, c, ik, 0, lo < 0 ? 0 : lo, &r.a0, &r.a1);
  if (hi < n) trim_range(b, c, ik, hi < 0 ? 0 : hi, n, &r.b0, &r.b1);
  return r;
}

// The storage ranges untrimmed (the switch that turns the trimming off).
inline ActiveRanges full_ranges(int n, int lo, int hi) {
  ActiveRanges r{0, lo > n ? n : lo, 0, 0};
  if (r.a1 <= 0) r.a0 = r.a1 = 0;
  if (hi < n) { r.b0 = hi; r.b1 = n; }
  return r;
}

// rows: nrows rows of `len` payload bytes, `stride` bytes apart.  On success ids[r] is the index of row r's pattern and pats holds the
// distinct rows back to back (len bytes each, in order of first appearance).  Gives up (false, outputs unspecified) as soon as the
// patterns would exceed max_bytes.
inline bool dedup_rows(const uint8_t* rows, size_t nrows, size_t len, size_t stride, size_t max_bytes, std::vector<int32_t>* ids,
                       std::vector<uint8_t>* pats) {
  ids->assign(nrows, 0);
  pats->clear();
  if (len == 0) return nrows == 0;
  std::unordered_map<std::string_view, int32_t> seen;   // keys view the caller's rows, which outlive the map
  for (size_t r = 0; r < nrows; ++r) {
    const std::string_view key(reinterpret_cast<const char*>(rows + r * stride), len);
    auto it = seen.find(key);
    if (it == seen.end()) {
      if ((seen.size() + 1) * len > max_bytes) return false;
      it = seen.emplace(key, (int32_t)seen.size()).first;
      pats->insert(pats->end(), rows + r * stride, rows + r * stride + len);
    }
    (*ids)[r] = it->second;
  }
  return true;
}

}   // namespace host_tables
