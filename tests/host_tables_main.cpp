// Stand-alone check of csrc/host_tables.hpp (no HIP, no Python): the CPML active-range trimming and the class-row dedup on synthetic
// tables.  Built by tests/test_host_tables_cpu.py with the host compiler, plain and with -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../fdtd-solver-antennas_amd/csrc/host_tables.hpp"

using host_tables::ActiveRanges;

static int g_failed = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
  } while (0)

struct Tables {
  std::vector<float> b, c, ik;
  explicit Tables(int n) : b(n, 0.f), c(n, 0.f), ik(n, 1.f) {}
  void on(int q) { b[q] = 0.5f; c[q] = -0.25f; ik[q] = 1.f; }
  ActiveRanges trim(int lo, int hi) const { return host_tables::trim_active(b.data(), c.data(), ik.data(), (int)b.size(), lo, hi); }
};
static bool eq(const ActiveRanges& r, int a0, int a1, int b0, int b1) { return r.a0 == a0 && r.a1 == a1 && r.b0 == b0 && r.b1 == b1; }

// the layout cpml.build_cpml gives an axis of n nodes with `lo` and `hi` layer cells: storage [0, lo) and [n - 1 - hi, n) (none if hi == 0);
// E-located inert: 0, n - 1 - hi, n - 1; H-located inert: n - 1
static void built_like(int n, int lo, int hi, bool h_side, Tables* t, int* slo, int* shi) {
  *slo = lo; *shi = hi ? n - 1 - hi : n;
  for (int q = 0; q < lo; ++q) if (h_side || q > 0) t->on(q);
  for (int q = n - 1 - hi + (h_side ? 0 : 1); hi && q < n - 1; ++q) t->on(q);
}

static void test_trim() {
  int lo, hi;
  {   // thickness 0: nothing stored, nothing active
    Tables t(12);
    CHECK(eq(t.trim(0, 12), 0, 0, 0, 0));
    CHECK(t.trim(0, 12).count() == 0 && host_tables::full_ranges(12, 0, 12).count() == 0);
  }
  {   // thickness 10 on both sides, E-located: 0, n - 11 and n - 1 go
    Tables t(40); built_like(40, 10, 10, false, &t, &lo, &hi);
    CHECK(lo == 10 && hi == 29);
    CHECK(eq(t.trim(lo, hi), 1, 10, 30, 39));
    CHECK(host_tables::full_ranges(40, lo, hi).count() - t.trim(lo, hi).count() == 3);
  }
  {   // ... H-located: the last index goes
    Tables t(40); built_like(40, 10, 10, true, &t, &lo, &hi);
    CHECK(eq(t.trim(lo, hi), 0, 10, 29, 39));
  }
  {   // thickness 1: the E side of the low layer has no active index at all; the high one keeps none either (n - 2 is where it begins)
    Tables t(9); built_like(9, 1, 1, false, &t, &lo, &hi);
    const ActiveRanges r = t.trim(lo, hi);
    CHECK(r.a0 == r.a1 && r.b0 == r.b1 && r.count() == 0);
    Tables h(9); built_like(9, 1, 1, true, &h, &lo, &hi);
    CHECK(eq(h.trim(lo, hi), 0, 1, 7, 8));
  }
  {   // one-sided: low layer only, high layer only
    Tables t(20); built_like(20, 4, 0, false, &t, &lo, &hi);
    CHECK(hi == 20 && eq(t.trim(lo, hi), 1, 4, 0, 0));
    Tables u(20); built_like(20, 0, 5, false, &u, &lo, &hi);
    CHECK(lo == 0 && hi == 14 && eq(u.trim(lo, hi), 0, 0, 15, 19));
  }
  {   // an inert index in the middle of a range stays active; only the ends are trimmed
    Tables t(30); built_like(30, 8, 6, true, &t, &lo, &hi);
    t.b[3] = 0.f; t.c[3] = 0.f; t.ik[3] = 1.f;
    t.b[25] = 0.f; t.c[25] = 0.f; t.ik[25] = 1.f;
    CHECK(eq(t.trim(lo, hi), 0, 8, 23, 29));
  }
  {   // -0.0f coefficients are inert; 1 / kappa != 1 alone, b alone or c alone keep an index active
    Tables t(16); built_like(16, 4, 4, true, &t, &lo, &hi);
    t.b[0] = -0.f; t.c[0] = -0.f; t.ik[0] = 1.f;
    t.b[1] = -0.f; t.c[1] = 0.f; t.ik[1] = 0.75f;
    CHECK(eq(t.trim(lo, hi), 1, 4, 11, 15));
    t.ik[1] = 1.f; t.c[1] = 1e-30f;
    CHECK(eq(t.trim(lo, hi), 1, 4, 11, 15));
    t.c[1] = -0.f; t.b[1] = 1e-30f;
    CHECK(eq(t.trim(lo, hi), 1, 4, 11, 15));
    t.b[1] = 0.f;
    CHECK(eq(t.trim(lo, hi), 2, 4, 11, 15));
  }
  {   // whole ranges inert; the switch that keeps everything
    Tables t(10);
    CHECK(t.trim(3, 6).count() == 0);
    const ActiveRanges f = host_tables::full_ranges(10, 3, 6);
    CHECK(eq(f, 0, 3, 6, 10) && f.count() == 7);
    CHECK(eq(host_tables::full_ranges(10, 3, 10), 0, 3, 0, 0));
    CHECK(eq(host_tables::full_ranges(10, 3, 1 << 30), 0, 3, 0, 0));
  }
}

static void test_dedup() {
  std::vector<int32_t> ids;
  std::vector<uint8_t> pats;
  {   // all rows equal; payload of 7 bytes in rows 8 bytes apart (the pad byte differs and must not count)
    const size_t nrows = 50, len = 7, stride = 8;
    std::vector<uint8_t> rows(nrows * stride);
    for (size_t r = 0; r < nrows; ++r) {
      for (size_t q = 0; q < len; ++q) rows[r * stride + q] = (uint8_t)(3 * q + 1);
      rows[r * stride + len] = (uint8_t)r;
    }
    CHECK(host_tables::dedup_rows(rows.data(), nrows, len, stride, 1 << 20, &ids, &pats));
    CHECK(pats.size() == len && ids.size() == nrows);
    for (size_t r = 0; r < nrows; ++r) CHECK(ids[r] == 0);
    for (size_t q = 0; q < len; ++q) CHECK(pats[q] == (uint8_t)(3 * q + 1));
  }
  {   // a few distinct rows, in order of first appearance; every row is reproduced by its pattern
    const size_t nrows = 200, len = 13, stride = 13;
    std::vector<uint8_t> rows(nrows * stride);
    for (size_t r = 0; r < nrows; ++r)
      for (size_t q = 0; q < len; ++q) rows[r * stride + q] = (uint8_t)((r * r) % 5 + (q == 12 ? 100 : 0));
    CHECK(host_tables::dedup_rows(rows.data(), nrows, len, stride, 1 << 20, &ids, &pats));
    CHECK(pats.size() == 3 * len);   // r * r mod 5 takes the values 0, 1, 4
    CHECK(ids[0] == 0 && ids[1] == 1 && ids[2] == 2 && ids[3] == 2 && ids[4] == 1 && ids[5] == 0);
    for (size_t r = 0; r < nrows; ++r) CHECK(memcmp(rows.data() + r * stride, pats.data() + (size_t)ids[r] * len, len) == 0);
  }
  {   // all rows different: beyond the limit the row form is refused (the caller keeps the per-cell bytes), within it it is exact
    const size_t nrows = 300, len = 16;
    std::vector<uint8_t> rows(nrows * len, 0);
    for (size_t r = 0; r < nrows; ++r) { rows[r * len] = (uint8_t)r; rows[r * len + 15] = (uint8_t)(r >> 8); }
    CHECK(!host_tables::dedup_rows(rows.data(), nrows, len, len, 299 * len, &ids, &pats));
    CHECK(host_tables::dedup_rows(rows.data(), nrows, len, len, 300 * len, &ids, &pats));
    CHECK(pats.size() == nrows * len);
    for (size_t r = 0; r < nrows; ++r) CHECK(ids[r] == (int32_t)r);
  }
  {   // nothing to do
    CHECK(host_tables::dedup_rows(nullptr, 0, 8, 8, 1 << 20, &ids, &pats) && ids.empty() && pats.empty());
  }
}

int main() {
  test_trim();
  test_dedup();
  if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
  printf("host_tables ok\n");
  return 0;
}
