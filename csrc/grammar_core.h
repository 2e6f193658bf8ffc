// The grammar walk (engine/grammar.py states the compiled form): ONE function, step(), holds the
// transition rule, and walk() advances (q, depth, stack) over a byte span with it. They compile for the
// host and the device: the mask kernel (grammar_mask.hip), its step hand-over and the host program
// csrc/tests/grammar_check.cpp all run this copy. No HIP calls, no
// environment reads. Every index read from a table is checked against the table's extent, so a
// corrupt table or state can make a walk dead but never read outside `trans` / `cls`.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GR_HD __host__ __device__ __forceinline__     // inlined, so a Table never has to live in scratch memory
#else
#define GR_HD inline
#endif

namespace gr {

constexpr int MAX_DEPTH = 32;          // grammar.GRAMMAR_MAX_DEPTH: the stack is one 32-bit word
constexpr int MAX_STATES = 4096;       // grammar.GRAMMAR_MAX_STATES
constexpr int MAX_CLASSES = 64;        // grammar.GRAMMAR_MAX_CLASSES
constexpr int MAX_TABLE = 65536;       // grammar.GRAMMAR_MAX_TABLE: entries of one row's table
constexpr int TOKEN_BYTE_CAP = 128;    // grammar.GRAMMAR_TOKEN_BYTE_CAP
constexpr int MAX_STOPS = 8;           // grammar.GRAMMAR_MAX_STOPS
constexpr int Q_FIN = -1, Q_DEAD = -2;
constexpr uint16_t DEAD_ENTRY = 0xFFFF;
constexpr int ACT_POP = 3;             // 0 none, 1 push 0 (object), 2 push 1 (array), 3 pop

struct State {
  int q, depth;
  uint32_t stack;     // bit i: container i (0 = object, 1 = array); bit depth - 1 is the top
};

// A row's automaton. `trans` [n_states * n_classes], `cls` [256]; they may point to global memory or LDS.
struct Table {
  const uint16_t* trans;
  const uint8_t* cls;
  int n_states, n_classes;
  // state after a pop with an object / an array / nothing then on top (-1: none). Three fields, not an
  // array: an array indexed at run time would send the whole struct to scratch memory on the device.
  int pop_obj, pop_arr, pop_empty;
};

// ONE transition: consume `byte` from (q, depth, stack), all three valid. False at a byte without a
// transition: no entry, a push at MAX_DEPTH, a pop on an empty stack, or an index outside the table.
GR_HD bool step(const Table& t, int& q, int& depth, uint32_t& stack, uint8_t byte) {
  const int c = t.cls[byte];
  if (c >= t.n_classes) return false;
  const uint16_t e = t.trans[q * t.n_classes + c];
  if (e == DEAD_ENTRY) return false;
  const int act = e & 3;
  if (act == ACT_POP) {
    if (depth == 0) return false;
    --depth;
    stack &= ~(1u << depth);
    // values, not `c ? t.a : t.b` on the fields: that selects an ADDRESS and keeps the Table in memory
    const int on_obj = t.pop_obj, on_arr = t.pop_arr, on_empty = t.pop_empty;
    q = depth == 0 ? on_empty : (((stack >> (depth - 1)) & 1u) ? on_arr : on_obj);
  } else {
    if (act != 0) {
      if (depth == MAX_DEPTH) return false;
      stack |= (uint32_t)(act - 1) << depth;
      ++depth;
    }
    q = e >> 2;
  }
  return q >= 0 && q < t.n_states;
}

GR_HD bool valid(const Table& t, const State& s) { return s.q >= 0 && s.q < t.n_states && s.depth >= 0 && s.depth <= MAX_DEPTH; }
GR_HD bool kill(State& s) { return s.q = Q_DEAD, s.depth = 0, s.stack = 0, false; }

// Advance `s` over data[0:n] with step(). Returns false (s = DEAD) at the first byte without a
// transition. FIN / DEAD stay. (The kernel's token loop calls step() itself, on bytes it fetches 16 at
// a time: grammar_mask.hip.)
GR_HD bool walk(const Table& t, State& s, const uint8_t* data, int n) {
  if (s.q < 0) return s.q == Q_FIN;
  if (!valid(t, s)) return kill(s);
  int q = s.q, depth = s.depth;
  uint32_t stack = s.stack;
  for (int i = 0; i < n; ++i)
    if (!step(t, q, depth, stack, data[i])) return kill(s);
  s.q = q, s.depth = depth, s.stack = stack;
  return true;
}

GR_HD bool is_stop(const int* stops, int n_stop, int64_t tok) {
  for (int i = 0; i < n_stop && i < MAX_STOPS; ++i)
    if (stops[i] == tok) return true;
  return false;
}

// The bytes of token `tok`, or n = 0 for an id outside [0, V), a zero-length token, a token over the
// byte cap or offsets that do not lie inside tok_bytes.
GR_HD const uint8_t* token_span(const int* tok_off, const uint8_t* tok_bytes, int64_t n_bytes, int V, int64_t tok,
                                int& n) {
  n = 0;
  if (tok < 0 || tok >= V) return tok_bytes;
  const int64_t a = tok_off[tok], b = tok_off[tok + 1];
  if (a < 0 || b <= a || b > n_bytes || b - a > TOKEN_BYTE_CAP) return tok_bytes;
  n = (int)(b - a);
  return tok_bytes + a;
}

// The state after consuming token `tok`: FIN and DEAD stay; a stop id gives FIN; a token with no
// usable bytes or a dead walk gives DEAD. (engine/grammar.py BoundGrammar.advance)
GR_HD void advance(const Table& t, State& s, const int* stops, int n_stop, const int* tok_off,
                   const uint8_t* tok_bytes, int64_t n_bytes, int V, int64_t tok) {
  if (s.q < 0) return;
  if (is_stop(stops, n_stop, tok)) { s.q = Q_FIN, s.depth = 0, s.stack = 0; return; }
  int n;
  const uint8_t* p = token_span(tok_off, tok_bytes, n_bytes, V, tok, n);
  if (n == 0) { s.q = Q_DEAD, s.depth = 0, s.stack = 0; return; }
  walk(t, s, p, n);
}

// ---- the token budget (engine/grammar.py GrammarBudget states the bound and why the rule is sound) ----
constexpr uint16_t NEED_INF16 = 0xFFFF;     // a 16-bit entry: no way through single-byte tokens
constexpr int NEED_INF = 1 << 30;           // need() with such an entry on its way
constexpr int BUDGET_FREE = 1 << 29;        // a budget that binds nothing

// A row's need arrays: c_acc[q] (to accept, at depth 0) and c_pop[q] (up to and including the next pop),
// n_states entries each, in global memory or on the host.
struct Need {
  const uint16_t* c_acc;
  const uint16_t* c_pop;
};

// An upper bound on the tokens that still lead from the live state (q, depth, stack) of table `t` to an
// accepting one: c_acc[q] at depth 0, else c_pop[q] + one c_pop[pop target] per stack level below the top
// (two popcounts) + c_acc[pop_empty]. NEED_INF when an entry it reads is NEED_INF16 or an index lies
// outside the table.
GR_HD int need(const Table& t, const Need& nd, int q, int depth, uint32_t stack) {
  if (q < 0 || q >= t.n_states || depth < 0 || depth > MAX_DEPTH) return NEED_INF;
  if (depth == 0) {
    const uint16_t a = nd.c_acc[q];
    return a == NEED_INF16 ? NEED_INF : (int)a;
  }
  const uint32_t below = (1u << (depth - 1)) - 1u;     // depth - 1 <= 31
  int ones = 0;
  for (uint32_t m = stack & below; m != 0; m &= m - 1) ++ones;
  const int zeros = depth - 1 - ones;
  const int on_obj = t.pop_obj, on_arr = t.pop_arr, on_empty = t.pop_empty;
  if (on_empty < 0 || on_empty >= t.n_states) return NEED_INF;
  const uint16_t p = nd.c_pop[q], e = nd.c_acc[on_empty];
  if (p == NEED_INF16 || e == NEED_INF16) return NEED_INF;
  int total = (int)p + (int)e;
  if (zeros > 0) {
    if (on_obj < 0 || on_obj >= t.n_states || nd.c_pop[on_obj] == NEED_INF16) return NEED_INF;
    total += zeros * (int)nd.c_pop[on_obj];
  }
  if (ones > 0) {
    if (on_arr < 0 || on_arr >= t.n_states || nd.c_pop[on_arr] == NEED_INF16) return NEED_INF;
    total += ones * (int)nd.c_pop[on_arr];
  }
  return total;     // at most 33 * 65534: no overflow
}

// Tokens the row may still emit, the one sampled now included: the row's budget less the device step.
GR_HD int remaining(int budget, int64_t step) {
  const int64_t r = (int64_t)budget - (step > 0 ? step : 0);
  return r < -1 ? -1 : (r > BUDGET_FREE ? BUDGET_FREE : (int)r);
}

// THE rule for a non-stop token whose walk stayed live: with r tokens left, one is kept back for the
// stop id and the document must still fit after this token. (r <= 0: nothing but stop ids.)
GR_HD bool budget_allows(int need_after, int r) { return r > 0 && need_after <= r - 2; }

// The free-phase shortcut: in a state whose flag says every token with bytes stays live, and with a
// budget no state's need can bind, the rule allows every token with bytes and no walk is needed.
GR_HD bool walks_skippable(bool all_live, int need_cap, int r) { return all_live && r > 0 && need_cap <= r - 2; }

}  // namespace gr
