// Budgeted grammar mask: grammar_mask.hip's mask under a per-row token budget, so a constrained reply
// ends with a stop id INSIDE max_new_tokens, and with a shortcut for the free phase of a `tail` grammar.
// Same place in the step (after the logit processors, before K6), same grid (B, chunks of V), one token
// per thread, same two-slot state hand-over by the kernel boundary alone; the walk is gr::step, the
// bound gr::need and the rule gr::budget_allows (grammar_core.h; engine/grammar.py GrammarBudget says
// why the rule never empties a row and always finishes).
//
// With r = budget[b] - *step tokens left for row b (the one sampled now included):
//  * a stop id is allowed exactly where grammar_mask.hip allows it;
//  * a non-stop token is allowed iff its walk stays live AND need(state after it) <= r - 2;
//  * r <= 0 is DEAD: stop ids only.
// Only a token whose walk survived reads the need arrays (a handful per workgroup in most states), so
// they stay in global memory and come through L2. A row without grammar_finish carries zero need arrays
// and budget BUDGET_FREE: the rule binds nothing and the result is grammar_mask.hip's, bit for bit.
//
// The row's state is advanced by thread 0 through the GLOBAL table before anything is staged, because
// the state decides whether to stage at all: in FIN / DEAD, and in a state flagged all-live with
// need_cap <= r - 2 (every token with bytes stays live and fits), no token is walked; the workgroup only
// stores -inf over byte-less tokens and stop ids and leaves. That is every step of a knight's free text.
// Otherwise the table is staged and walked as in grammar_mask.hip (placement rule: grammar_plan.h).
#include "common.h"
#include "grammar_plan.h"

namespace {
using namespace rt;

struct GrammarBudgetArgs {
  void* logits;
  int64_t ld;
  int V;
  const int* meta;           // [rows][META]; meta[7] = need_cap
  const uint8_t* cls;        // [rows][256]
  const uint16_t* tab;       // [rows][tab_entries]
  int tab_entries;
  const uint8_t* accept;     // [rows][state_cap]
  int state_cap;
  const int* stops;          // [rows][MAX_STOPS]
  int* state;                // [2][rows][STATE]
  int rows;
  const int* tok_off;        // [V + 1]
  const uint8_t* tok_bytes;  // [n_bytes], 16-byte aligned, n_bytes a multiple of 16
  int64_t n_bytes;
  const int64_t* out;        // [max_steps][out_ld] device-side token record, or nullptr
  const int64_t* step;       // device step counter, or nullptr (state from slot 0, r = budget)
  int max_steps;
  int out_ld;
  const int* budget;         // [rows]
  const uint16_t* c_acc;     // [rows][need_states]
  const uint16_t* c_pop;     // [rows][need_states]
  int need_states;
  const uint8_t* all_live;   // [rows][flag_states]
  int flag_states;
};

// One token per thread, walked as grammar_mask.hip walks it (bytes 16 at a time, the next 16 requested
// before these are walked); a survivor then has to fit the budget.
template <typename T>
RT_DEVICE void mask_token(const GrammarBudgetArgs& a, const gr::Table& t, const gr::Need& nd, const gr::State cur, int r,
                          bool stop_ok, const int* stops, int n_stop, T* row) {
  const int tok = blockIdx.y * gr::NT + threadIdx.x;
  if (tok >= a.V) return;
  bool allow;
  if (gr::is_stop(stops, n_stop, tok)) {
    allow = stop_ok;
  } else {
    int n;
    const uint8_t* p = gr::token_span(a.tok_off, a.tok_bytes, a.n_bytes, a.V, tok, n);
    allow = n > 0;
    if (allow) {
      const int lo = (int)(p - a.tok_bytes), hi = lo + n;
      const uint4* chunks = reinterpret_cast<const uint4*>(a.tok_bytes);
      int at = lo >> 4;
      uint4 nxt = chunks[at];
      int q = cur.q, depth = cur.depth;
      uint32_t stack = cur.stack;
      for (int pos = at << 4; allow && pos < hi; pos += 16) {
        const uint4 c = nxt;
        if (pos + 16 < hi) nxt = chunks[++at];
        const uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (allow && pos + k >= lo && pos + k < hi)
            allow = gr::step(t, q, depth, stack, (uint8_t)(w[k >> 2] >> ((k & 3) * 8)));
      }
      if (allow) allow = gr::budget_allows(gr::need(t, nd, q, depth, stack), r);
    }
  }
  if (!allow) DT<T>::store(row + tok, -INFINITY);
}

template <typename T>
__global__ void __launch_bounds__(gr::NT) grammar_budget_kernel(GrammarBudgetArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t s_tab[gr::LDS_ENTRIES];
  __shared__ uint8_t s_cls[256];
  __shared__ int s_stops[gr::MAX_STOPS];
  __shared__ int s_state[gr::STATE + 2];     // q, depth, stack, pad, r, no-walk
  const int b = blockIdx.x, tid = threadIdx.x;
  const int* m = a.meta + (size_t)b * gr::META;
  if (m[0] == 0) return;     // no grammar on this row (uniform: no barrier passed, nothing written)

  int ns = min(max(m[1], 0), a.state_cap), nc = min(max(m[2], 0), gr::MAX_CLASSES);
  if ((int64_t)ns * nc > a.tab_entries) ns = 0;     // a table that does not fit its slot: every state is dead
  const int entries = ns * nc;
  const int n_stop = min(max(m[6], 0), gr::MAX_STOPS);
  const uint16_t* gtab = a.tab + (size_t)b * a.tab_entries;
  const uint8_t* gcls = a.cls + (size_t)b * 256;
  const int* gstops = a.stops + (size_t)b * gr::MAX_STOPS;

  gr::Table t;
  t.trans = gtab;
  t.cls = gcls;
  t.n_states = ns, t.n_classes = nc;
  t.pop_obj = m[3], t.pop_arr = m[4], t.pop_empty = m[5];

  if (tid == 0) {     // the row's current state and budget: every workgroup of the row computes the same ones
    const int64_t s = a.step != nullptr ? *a.step : 0;
    gr::State st;
    if (s < 0 || s > a.max_steps) {
      st.q = gr::Q_DEAD, st.depth = 0, st.stack = 0;     // outside the record: stop ids only
    } else {
      const int* src = a.state + ((size_t)(s > 0 ? (s - 1) & 1 : 0) * a.rows + b) * gr::STATE;
      st.q = src[0], st.depth = src[1], st.stack = (uint32_t)src[2];
      if (s > 0) {
        gr::advance(t, st, gstops, n_stop, a.tok_off, a.tok_bytes, a.n_bytes, a.V, a.out[(size_t)(s - 1) * a.out_ld + b]);
        if (blockIdx.y == 0) {
          int* dst = a.state + ((size_t)(s & 1) * a.rows + b) * gr::STATE;
          dst[0] = st.q, dst[1] = st.depth, dst[2] = (int)st.stack, dst[3] = 0;
        }
      }
    }
    if (st.q >= ns || st.depth < 0 || st.depth > gr::MAX_DEPTH) st.q = gr::Q_DEAD;
    const int r = gr::remaining(a.budget[b], s);
    if (r <= 0 && st.q >= 0) st.q = gr::Q_DEAD;     // an exhausted budget masks like DEAD (the stored state is kept)
    const bool skip = st.q < 0 || gr::walks_skippable(a.all_live[(size_t)b * a.flag_states + st.q] != 0, m[7], r);
    s_state[0] = st.q, s_state[1] = st.depth, s_state[2] = (int)st.stack, s_state[4] = r, s_state[5] = skip;
  }
  __syncthreads();

  gr::State cur;
  cur.q = s_state[0], cur.depth = s_state[1], cur.stack = (uint32_t)s_state[2];
  const int r = s_state[4];
  const bool stop_ok = cur.q < 0 || a.accept[(size_t)b * a.state_cap + cur.q] != 0;
  T* row = reinterpret_cast<T*>(a.logits) + (size_t)b * a.ld;
  if (s_state[5] != 0) {     // uniform over the workgroup: nothing staged, no token walked
    const int tok = blockIdx.y * gr::NT + tid;
    if (tok >= a.V) return;
    bool allow;
    if (gr::is_stop(gstops, n_stop, tok)) {
      allow = stop_ok;
    } else {
      int n;
      gr::token_span(a.tok_off, a.tok_bytes, a.n_bytes, a.V, tok, n);
      allow = cur.q >= 0 && n > 0;
    }
    if (!allow) DT<T>::store(row + tok, -INFINITY);
    return;
  }

  const bool staged = entries <= gr::LDS_ENTRIES;
  if (staged) {     // 16 bytes per lane; the slot and s_tab are multiples of 8 entries, so the tail stays inside both
    const uint4* src = reinterpret_cast<const uint4*>(gtab);
    uint4* dst = reinterpret_cast<uint4*>(s_tab);
    for (int i = tid; i < (entries + 7) / 8; i += gr::NT) dst[i] = src[i];
  }
  s_cls[tid] = gcls[tid];     // NT == 256
  if (tid < gr::MAX_STOPS) s_stops[tid] = gstops[tid];
  __syncthreads();

  gr::Need nd;
  nd.c_acc = a.c_acc + (size_t)b * a.need_states;
  nd.c_pop = a.c_pop + (size_t)b * a.need_states;
  t.cls = s_cls;
  if (staged) {     // two copies, so each knows its table's address space (LDS reads, not flat ones)
    t.trans = s_tab;
    mask_token<T>(a, t, nd, cur, r, stop_ok, s_stops, n_stop, row);
  } else {
    t.trans = gtab;
    mask_token<T>(a, t, nd, cur, r, stop_ok, s_stops, n_stop, row);
  }
}
}  // namespace

// launch_grammar_mask's operands (grammar_mask.hip), then per row: budget int32 [budget_rows], the need
// arrays c_acc / c_pop [rows][need_states], the all-live flags [rows][flag_states]; need_cap is meta[7].
// Every refusal (grammar_plan.h) is returned before any HIP call.
int launch_grammar_mask_budget(void* logits, int dtype, int B, int V, int64_t ld, const int* meta, const uint8_t* cls,
                               const uint16_t* tab, int tab_entries, const uint8_t* accept, int state_cap,
                               int n_classes_cap, int byte_cap, const int* stops, int* state, int rows,
                               const int* tok_off, int64_t n_off, const uint8_t* tok_bytes, int64_t n_bytes,
                               const int64_t* out, const int64_t* step, int max_steps, int out_ld, const int* budget,
                               int budget_rows, const uint16_t* c_acc, const uint16_t* c_pop, int need_states,
                               const uint8_t* all_live, int flag_states, hipStream_t stream) {
  if (B <= 0) return 0;
  const gr::MaskPlan pl =
      gr::plan_grammar_budget(B, V, ld, dtype, tab_entries, state_cap, n_classes_cap, byte_cap, n_off, n_bytes, rows,
                              out != nullptr, step != nullptr, max_steps, out_ld, need_states, flag_states, budget_rows);
  if (pl.rc != 0) return pl.rc;
  if (logits == nullptr || meta == nullptr || cls == nullptr || tab == nullptr || accept == nullptr ||
      stops == nullptr || state == nullptr || tok_off == nullptr || tok_bytes == nullptr || budget == nullptr ||
      c_acc == nullptr || c_pop == nullptr || all_live == nullptr ||
      (reinterpret_cast<uintptr_t>(tok_bytes) & 15) != 0 || (reinterpret_cast<uintptr_t>(tab) & 15) != 0)
    return -11;     // a null operand, or token bytes / tables not 16-byte aligned
  GrammarBudgetArgs a{logits,  ld,        V,         meta,    cls, tab,  tab_entries, accept, state_cap,
                      stops,   state,     rows,      tok_off, tok_bytes, n_bytes,     out,    step,
                      max_steps, out_ld,  budget,    c_acc,   c_pop, need_states, all_live, flag_states};
  const dim3 grid(B, pl.chunks);
  if (dtype == 0)
    hipLaunchKernelGGL(grammar_budget_kernel<uint16_t>, grid, dim3(gr::NT), 0, stream, a);
  else
    hipLaunchKernelGGL(grammar_budget_kernel<float>, grid, dim3(gr::NT), 0, stream, a);
  return 0;
}
