// Host-side plan of the logprob launches (logprobs.hip): the chunk count, the workspace layout and
// the refusals — a pure function of the shape. No HIP calls, no device code and no environment
// reads, so a host program can exercise every rule without a GPU.
#pragma once
#include <cstdint>

namespace lpr {

constexpr int MAX_TOP = 20;        // ops.MAX_TOP_LOGPROBS: alternatives a row can ask for
constexpr int CHUNK = 4096;        // elements per workgroup of logprob_chunks, fixed
constexpr int MAX_CHUNKS = 64;     // V <= 64 * 4096
// workspace words of one (row, chunk): max, sum exp(l - max), count, pad, 20 keys, 20 ids.
// 44 words = 11 x 16 bytes; a row always owns MAX_CHUNKS records, whatever V is, so one
// allocation serves every vocabulary.
constexpr int WS_M = 0, WS_S = 1, WS_N = 2, WS_KEY = 4, WS_ID = WS_KEY + MAX_TOP;
constexpr int WS_REC = WS_ID + MAX_TOP;
constexpr int WS_ROW = MAX_CHUNKS * WS_REC;
static_assert(WS_REC % 4 == 0, "records start 16-byte aligned");

inline int64_t workspace_words(int B) { return (int64_t)(B > 0 ? B : 0) * WS_ROW; }

struct LogprobPlan {
  int rc = 0;      // 0, or -1 V / ld, -2 V > MAX_CHUNKS * CHUNK, -3 dtype, -4 record narrower than MAX_TOP
                   // columns, -5 out without step or the reverse (or neither and no ids), -6 out_ld < B,
                   // -7 records do not cover the batch / the steps, -8 workspace too small
  int nch = 0;     // chunks per row = grid.y of logprob_chunks
};

// dtype: 0 = bf16, 1 = fp32. rec_cols: columns of top_id / top_lp; rec_ld: rows of a record step
// (>= B); rec_steps: record steps. Graph form: has_out && has_step (then max_steps record steps are
// written); eager form: has_ids, neither out nor step.
inline LogprobPlan plan_logprobs(int B, int V, int64_t ld, int dtype, int rec_cols, int rec_ld, int rec_steps,
                                 bool has_ids, bool has_out, bool has_step, int max_steps, int out_ld,
                                 int64_t ws_words) {
  LogprobPlan pl;
  if (V <= 0 || ld < V) return pl.rc = -1, pl;
  if (V > MAX_CHUNKS * CHUNK) return pl.rc = -2, pl;
  if (dtype != 0 && dtype != 1) return pl.rc = -3, pl;
  if (rec_cols < MAX_TOP) return pl.rc = -4, pl;
  if (has_out != has_step || (!has_out && !has_ids)) return pl.rc = -5, pl;
  if (has_out && out_ld < B) return pl.rc = -6, pl;
  if (rec_ld < B || rec_steps < 1 || (has_out && (max_steps < 0 || rec_steps < max_steps))) return pl.rc = -7, pl;
  if (ws_words < workspace_words(B)) return pl.rc = -8, pl;
  pl.nch = (V + CHUNK - 1) / CHUNK;
  return pl;
}

}  // namespace lpr
