// corrections.hpp — the step-loop corrections as one table: what api.hip knows of a correction is its row, and nothing else.
//
// A correction is a launch between the E phase and the H update (E side), behind the H update (H side), or both.  Its .hip file defines
// the kernel, the exported set / get functions and ONE row next to the functions the row points at; api.hip walks the table for the
// launches, the planner's questions, the refusals, the teardown and the re-priming.  Adding a correction is adding a row.
#pragma once
#include "fdtd_ctx.h"

struct CorrectionRow {
  const char* name;                                   // as the refusals spell it
  bool no_links;                                      // linked contexts are refused besides decomposed grids and the p2p transport
  bool volume;                                        // a volume of edges (ports sit inside it): the V-probes always go in front
  bool (*active)(const fdtd_ctx*);                    // a non-empty set is in place
  void (*launch_E)(fdtd_ctx*, long long step, hipStream_t);   // behind the E phase, in front of the H update (null: none; a no-op while inactive)
  void (*launch_H)(fdtd_ctx*, long long step, hipStream_t);   // behind the H update, in front of whatever reads I next (likewise)
  void (*release)(fdtd_ctx*);                         // the set's device memory and host state (leaves the correction inactive)
  const EdgeFacts* (*edge_facts)(const fdtd_ctx*);    // a sparse E-side list: what the planner asks of its edges (null: none)
  int (*prime)(fdtd_ctx*, int comp);                  // after fdtd_set_field(FDTD_KIND_I, comp): re-derive the state kept of I (null: none)
};

// A row holds addresses of host functions: its definition stands inside #ifndef __HIP_DEVICE_COMPILE__, or the device pass of its file
// would emit the constant, and with it device copies of those functions.
// The table's order is the order of the REFUSALS (plan_schedule names the first active correction it cannot step) — not of the launches
enum Correction { CORR_SHEET, CORR_DEBYE, CORR_LORENTZ, CORR_LUMPED, CORR_MAGNETIC, CORR_CONFORMAL, CORR_PLANEWAVE, CORR_EXCITE, CORR_COUNT };
extern const CorrectionRow corr_sheet, corr_debye, corr_lorentz, corr_lumped, corr_magnetic, corr_conformal, corr_planewave, corr_excite;
inline const CorrectionRow* const corrections[] = {&corr_sheet, &corr_debye, &corr_lorentz, &corr_lumped,
                                                   &corr_magnetic, &corr_conformal, &corr_planewave, &corr_excite};
static_assert(sizeof(corrections) / sizeof(corrections[0]) == CORR_COUNT, "one row per enum Correction");
// The two launch orders (the headers' order: volumes, then the sparse lists; the incident field last of either side but for the excitations)
constexpr Correction launch_order_E[] = {CORR_DEBYE, CORR_LORENTZ, CORR_SHEET, CORR_LUMPED, CORR_PLANEWAVE};
constexpr Correction launch_order_H[] = {CORR_MAGNETIC, CORR_CONFORMAL, CORR_PLANEWAVE, CORR_EXCITE};

// What the planner keeps of a list of edges given by their local offsets (EdgeFacts, fdtd_ctx.h).  (Lists exist on single slabs only.)
inline EdgeFacts edge_facts_of(const fdtd_ctx* c, std::vector<int> off) {
  EdgeFacts f;
  const int nn[3] = {c->d.nx, c->d.ny, c->d.nz};
  for (const int o : off) {
    const int k = o / c->plane, j = (o - k * c->plane) / c->P;
    const int pos[3] = {o - k * c->plane - j * c->P, j, k + c->d.k0};
    for (int a = 0; a < 3; ++a) f.faces |= (pos[a] == 0 ? 1u : 0u) << (2 * a) | (pos[a] == nn[a] - 1 ? 1u : 0u) << (2 * a + 1);
  }
  std::sort(off.begin(), off.end());
  f.h_off = std::move(off);
  return f;
}

// ---- what the set functions share ---------------------------------------------------------------------------------------------------
// FDTD_OK, or the refusal of a decomposed / p2p / linked context
inline int correction_single_slab(fdtd_ctx* c, const CorrectionRow& k) {
  if (c->d.world > 1 || c->p.p2p || (k.no_links && (c->link_lo || c->link_hi)))
    return fdtd_fail(c, FDTD_E_UNSUPPORTED, k.no_links ? "%s: single slab only (world = 1, no p2p transport, no linked contexts)" : "%s: single slab only (world = 1)", k.name);
  return FDTD_OK;
}
inline int correction_set_state(fdtd_ctx* c, const char* who) {
  if (!c->have_op) return fdtd_fail(c, FDTD_E_STATE, "%s: set the operator first", who);
  if (c->step != 0) return fdtd_fail(c, FDTD_E_STATE, "%s: before the first timestep", who);
  return FDTD_OK;
}
// behind the argument checks, in front of the validation of the set's contents: a non-empty set needs a single slab, any set the operator and step 0
inline int correction_set_begin(fdtd_ctx* c, const CorrectionRow& k, const char* who, bool nonempty) {
  if (nonempty)
    if (int r = correction_single_slab(c, k)) return r;
  return correction_set_state(c, who);
}
// behind the validation: nothing in flight reads the old set, which goes
inline int correction_set_replace(fdtd_ctx* c, const CorrectionRow& k) {
  HIPCK(c, hipSetDevice(c->d.device));
  HIPCK(c, hipStreamSynchronize(c->stream));
  k.release(c);
  return FDTD_OK;
}
// an allocation or copy of the new set failed: no half a set stays
inline int correction_set_failed(fdtd_ctx* c, const CorrectionRow& k, const char* who, hipError_t e) {
  k.release(c);
  return fdtd_fail_hip(c, who, e);
}
// sheet.hip, shared with lumped.hip: the list's prologue (state checks, every edge inside the grid and existing, classes in range, no
// edge twice; then the stream synchronised, the row's old set released, the list's arrays uploaded, the planner's facts kept) and its release
int edge_list_set(fdtd_ctx* c, EdgeList* l, const CorrectionRow& row, const char* who, int n, const int64_t* idx, const int8_t* comp,
                  const float* vi, const int32_t* cls, int ncls);
void edge_list_free(EdgeList* l);
