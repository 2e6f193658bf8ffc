// Host-side plan of the grammar mask launch (grammar_mask.hip): the grid, the
// table placement rule and the refusals — a pure function of the shape. No HIP calls, no device code
// and no environment reads, so a host program can exercise every rule without a GPU.
#pragma once
#include <cstdint>

#include "grammar_core.h"

namespace gr {

constexpr int NT = 256;               // threads per workgroup = consecutive ids it masks, one token per thread
constexpr int MAX_V = 1 << 20;        // vocabulary sizes the kernel is tested for
// A row's table is staged in LDS when it has at most this many entries (32 KiB; json_object has about
// 3.3K, the schemas of the tests 5-10K), else every lookup goes through L2 (a schema with a 40-character
// string has 40K; measured, the two placements are within 10% of each other). The rule is per row and
// taken on the device from the row's own n_states * n_classes: a captured launch is refilled with
// other grammars, so the host cannot fix the placement at launch time.
constexpr int LDS_ENTRIES = 16384;
constexpr int META = 8;               // ints per row: active, n_states, n_classes, pop obj/arr/empty, n_stop, pad
constexpr int STATE = 4;              // ints per (slot, row): q, depth, stack, pad

struct MaskPlan {
  int rc = 0;       // 0, or -1 V / ld, -2 V > MAX_V, -3 dtype, -4 table slot (8..MAX_TABLE entries, a multiple of
                    // 8: the kernel stages 16 bytes per lane) or accept slot (1..MAX_STATES), -5 classes,
                    // -6 token byte cap, -7 out without step or the reverse, -8 out_ld < B / max_steps < 0,
                    // -9 token table: fewer than V + 1 offsets, or bytes not a positive multiple of 16 (the kernel
                    // fetches them 16 at a time), -10 per-row operands do not cover B
  int chunks = 0;   // grid.y: workgroups per row
};

// tab_entries: entries each row's table slot holds; state_cap: states `accept` holds per row; n_off: length of
// tok_off; rows: rows the per-row operands (meta, cls, tab, accept, stops, state) cover.
inline MaskPlan plan_grammar_mask(int B, int V, int64_t ld, int dtype, int tab_entries, int state_cap, int n_classes_cap,
                                  int byte_cap, int64_t n_off, int64_t n_bytes, int rows, bool has_out, bool has_step,
                                  int max_steps, int out_ld) {
  MaskPlan pl;
  if (V <= 0 || ld < V) return pl.rc = -1, pl;
  if (V > MAX_V) return pl.rc = -2, pl;
  if (dtype != 0 && dtype != 1) return pl.rc = -3, pl;
  if (tab_entries < 8 || tab_entries % 8 != 0 || tab_entries > MAX_TABLE || state_cap < 1 || state_cap > MAX_STATES) return pl.rc = -4, pl;
  if (n_classes_cap < 1 || n_classes_cap > MAX_CLASSES) return pl.rc = -5, pl;
  if (byte_cap != TOKEN_BYTE_CAP) return pl.rc = -6, pl;
  if (has_out != has_step) return pl.rc = -7, pl;
  if (has_out && (out_ld < B || max_steps < 0)) return pl.rc = -8, pl;
  if (n_off < (int64_t)V + 1 || n_bytes < 16 || n_bytes % 16 != 0) return pl.rc = -9, pl;
  if (rows < B) return pl.rc = -10, pl;
  pl.chunks = (V + NT - 1) / NT;
  return pl;
}

// The budgeted launch (grammar_budget.hip) takes the same shape and, per row, budget int32, the two need
// arrays c_acc / c_pop [rows][need_cap_states] of 16-bit entries, the all-live flags [rows][flag_states]
// and need_cap in meta[7]. Its refusals are the plain launch's, then -12: the need arrays or the flags
// do not hold a row's state_cap states, or the budget does not cover `rows`.
inline MaskPlan plan_grammar_budget(int B, int V, int64_t ld, int dtype, int tab_entries, int state_cap, int n_classes_cap,
                                    int byte_cap, int64_t n_off, int64_t n_bytes, int rows, bool has_out, bool has_step,
                                    int max_steps, int out_ld, int need_states, int flag_states, int budget_rows) {
  MaskPlan pl = plan_grammar_mask(B, V, ld, dtype, tab_entries, state_cap, n_classes_cap, byte_cap, n_off, n_bytes, rows,
                                  has_out, has_step, max_steps, out_ld);
  if (pl.rc != 0) return pl;
  if (need_states < state_cap || flag_states < state_cap || budget_rows < rows) return pl.rc = -12, pl.chunks = 0, pl;
  return pl;
}

}  // namespace gr
