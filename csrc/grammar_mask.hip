// Grammar mask: sets the logits of the tokens a row's grammar cannot accept next to -inf, in place,
// AFTER the logit processors (logit_proc.hip) and BEFORE K6 (sampling.hip) samples. One launch per step.
//
// The automaton (engine/grammar.py) works on bytes; a row's state is (q, depth, stack). A token is
// allowed when the walk (grammar_core.h) over its bytes from the row's CURRENT state does not die; a
// stop id is allowed exactly in an accepting state and in FIN / DEAD, where nothing else is: such a row
// always keeps its stop ids finite, so no row leaves this kernel without a finite element (the host
// refuses a (grammar, tokenizer) pair in which a live state allows no token: BoundGrammar).
//
// Grid (B, chunks of V); a workgroup masks NT consecutive ids of one row, one token per thread, so
// the lanes of a wave store to neighbouring elements. Disallowed elements get
// one plain 2- or 4-byte vector store of -inf; allowed elements are never written and keep their
// bits. Nothing at or past column V is touched. A row without a grammar returns before any barrier.
//
// Step hand-over in a captured graph — no ticket, no last arriver, only the kernel boundary: the state
// lives in a two-slot buffer state[2][rows][4]. At *step = s > 0 EVERY workgroup of row b reads slot
// (s - 1) & 1 and advances it over the token K6 recorded at out[s - 1, b]; the row's workgroup 0 stores
// the result to slot s & 1, which no workgroup of this launch reads (the next launch does, after the
// boundary). At s = 0, and on the eager path (step == nullptr), the state is what the host put in slot 0.
// The advance is one token's walk by one thread (a few LDS lookups), so it stays in this launch: a
// launch of its own would add a kernel boundary (> 1 µs) to save that.
//
// Choices (profiles/r11/grammar/README.md has the figures):
//  * table placement: the walk is a chain of dependent lookups, cls[byte] then trans[q][class]; from
//    LDS a link costs about 2 x 50 cycles, through L2 several times that. A row's table is staged in
//    LDS when it fits LDS_ENTRIES (grammar_plan.h); the 256-byte class map always is. A larger table
//    is read through L2 — same result, and measured within 10% of the staged time: most tokens die
//    at their first byte, and the launch is not bound by the lookups.
//  * tokens per thread: 1. Builds that gave a thread 2, 4 or 8 tokens, walked one after the other, took
//    27 / 37 / 58 µs against 22 µs (B = 3, V = 128256, json_object at its start state): the staging a
//    wider workgroup would share is small beside that.
//  * token order: id order. Walks are very uneven (a token dies at its first byte in most JSON states
//    and runs to its end inside a string), but lengths are not correlated with ids inside a chunk,
//    and sorting tokens by length would scatter the -inf stores and need a per-tokenizer permutation.
#include "common.h"
#include "grammar_plan.h"

namespace {
using namespace rt;

struct GrammarMaskArgs {
  void* logits;
  int64_t ld;
  int V;
  const int* meta;           // [rows][META]
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
  const int64_t* step;       // device step counter, or nullptr (state from slot 0)
  int max_steps;
  int out_ld;
};

// One token per thread: token blockIdx.y * NT + threadIdx.x of the row.
template <typename T>
RT_DEVICE void mask_token(const GrammarMaskArgs& a, const gr::Table& t, const gr::State cur, bool stop_ok,
                          const int* stops, int n_stop, T* row) {
  const int tok = blockIdx.y * gr::NT + threadIdx.x;
  if (tok >= a.V) return;
  bool allow;
  if (gr::is_stop(stops, n_stop, tok)) {
    allow = stop_ok;
  } else if (cur.q < 0) {
    allow = false;
  } else {
    int n;
    const uint8_t* p = gr::token_span(a.tok_off, a.tok_bytes, a.n_bytes, a.V, tok, n);
    allow = n > 0;
    if (allow) {
      // The token's bytes come 16 at a time (aligned; tok_bytes is a multiple of 16 long), the next 16
      // requested before these are walked, so no byte load sits inside the chain of dependent lookups.
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
    }
  }
  if (!allow) DT<T>::store(row + tok, -INFINITY);
}

template <typename T>
__global__ void __launch_bounds__(gr::NT) grammar_mask_kernel(GrammarMaskArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t s_tab[gr::LDS_ENTRIES];
  __shared__ uint8_t s_cls[256];
  __shared__ int s_stops[gr::MAX_STOPS];
  __shared__ int s_state[gr::STATE];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int* m = a.meta + (size_t)b * gr::META;
  if (m[0] == 0) return;     // no grammar on this row (uniform: no barrier passed, nothing written)

  int ns = min(max(m[1], 0), a.state_cap), nc = min(max(m[2], 0), gr::MAX_CLASSES);
  if ((int64_t)ns * nc > a.tab_entries) ns = 0;     // a table that does not fit its slot: every state is dead
  const int entries = ns * nc;
  const int n_stop = min(max(m[6], 0), gr::MAX_STOPS);
  const uint16_t* gtab = a.tab + (size_t)b * a.tab_entries;
  const bool staged = entries <= gr::LDS_ENTRIES;
  if (staged) {     // 16 bytes per lane; the slot and s_tab are multiples of 8 entries, so the tail stays inside both
    const uint4* src = reinterpret_cast<const uint4*>(gtab);
    uint4* dst = reinterpret_cast<uint4*>(s_tab);
    for (int i = tid; i < (entries + 7) / 8; i += gr::NT) dst[i] = src[i];
  }
  s_cls[tid] = a.cls[(size_t)b * 256 + tid];     // NT == 256
  if (tid < gr::MAX_STOPS) s_stops[tid] = a.stops[(size_t)b * gr::MAX_STOPS + tid];
  __syncthreads();

  gr::Table t;
  t.trans = staged ? s_tab : gtab;
  t.cls = s_cls;
  t.n_states = ns, t.n_classes = nc;
  t.pop_obj = m[3], t.pop_arr = m[4], t.pop_empty = m[5];

  if (tid == 0) {     // the row's current state: every workgroup of the row computes the same one
    int64_t s = a.step != nullptr ? *a.step : 0;
    gr::State st;
    if (s < 0 || s > a.max_steps) {
      st.q = gr::Q_DEAD, st.depth = 0, st.stack = 0;     // outside the record: stop ids only
    } else {
      const int* src = a.state + ((size_t)(s > 0 ? (s - 1) & 1 : 0) * a.rows + b) * gr::STATE;
      st.q = src[0], st.depth = src[1], st.stack = (uint32_t)src[2];
      if (s > 0) {
        gr::advance(t, st, s_stops, n_stop, a.tok_off, a.tok_bytes, a.n_bytes, a.V, a.out[(size_t)(s - 1) * a.out_ld + b]);
        if (blockIdx.y == 0) {
          int* dst = a.state + ((size_t)(s & 1) * a.rows + b) * gr::STATE;
          dst[0] = st.q, dst[1] = st.depth, dst[2] = (int)st.stack, dst[3] = 0;
        }
      }
    }
    if (st.q >= ns || st.depth < 0 || st.depth > gr::MAX_DEPTH) st.q = gr::Q_DEAD;
    s_state[0] = st.q, s_state[1] = st.depth, s_state[2] = (int)st.stack;
  }
  __syncthreads();

  gr::State cur;
  cur.q = s_state[0], cur.depth = s_state[1], cur.stack = (uint32_t)s_state[2];
  const bool stop_ok = cur.q < 0 || a.accept[(size_t)b * a.state_cap + cur.q] != 0;
  T* row = reinterpret_cast<T*>(a.logits) + (size_t)b * a.ld;
  if (staged) {     // two copies, so each knows its table's address space (LDS reads, not flat ones)
    t.trans = s_tab;
    mask_token<T>(a, t, cur, stop_ok, s_stops, n_stop, row);
  } else {
    t.trans = gtab;
    mask_token<T>(a, t, cur, stop_ok, s_stops, n_stop, row);
  }
}
}  // namespace

// dtype: 0 = bf16, 1 = fp32 logits [B, V], row stride ld. Per-row operands cover `rows` >= B rows.
// Every refusal (grammar_plan.h) is returned before any HIP call.
int launch_grammar_mask(void* logits, int dtype, int B, int V, int64_t ld, const int* meta, const uint8_t* cls,
                        const uint16_t* tab, int tab_entries, const uint8_t* accept, int state_cap, int n_classes_cap,
                        int byte_cap, const int* stops, int* state, int rows, const int* tok_off, int64_t n_off,
                        const uint8_t* tok_bytes, int64_t n_bytes, const int64_t* out, const int64_t* step,
                        int max_steps, int out_ld, hipStream_t stream) {
  if (B <= 0) return 0;
  const gr::MaskPlan pl = gr::plan_grammar_mask(B, V, ld, dtype, tab_entries, state_cap, n_classes_cap, byte_cap, n_off,
                                                n_bytes, rows, out != nullptr, step != nullptr, max_steps, out_ld);
  if (pl.rc != 0) return pl.rc;
  if (logits == nullptr || meta == nullptr || cls == nullptr || tab == nullptr || accept == nullptr ||
      stops == nullptr || state == nullptr || tok_off == nullptr || tok_bytes == nullptr ||
      (reinterpret_cast<uintptr_t>(tok_bytes) & 15) != 0 || (reinterpret_cast<uintptr_t>(tab) & 15) != 0)
    return -11;     // a null operand, or token bytes / tables not 16-byte aligned
  GrammarMaskArgs a{logits, ld,   V,       meta,  cls,       tab,     tab_entries, accept,    state_cap, stops,
                    state,  rows, tok_off, tok_bytes, n_bytes, out, step, max_steps, out_ld};
  const dim3 grid(B, pl.chunks);
  if (dtype == 0)
    hipLaunchKernelGGL(grammar_mask_kernel<uint16_t>, grid, dim3(gr::NT), 0, stream, a);
  else
    hipLaunchKernelGGL(grammar_mask_kernel<float>, grid, dim3(gr::NT), 0, stream, a);
  return 0;
}
