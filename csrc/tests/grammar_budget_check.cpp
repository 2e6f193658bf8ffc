// Host check of the budgeted grammar mask's host-visible parts, without a GPU: need(), remaining(),
// budget_allows() and walks_skippable() of csrc/grammar_core.h (the copies the kernel runs) against
// cases the Python side wrote, the refusals of plan_grammar_budget (csrc/grammar_plan.h), and the
// launcher's argument validation, which must reject before any HIP call. Reads one file of
// whitespace-separated integers (tests/test_grammar_budget_host_check.py writes it and documents the
// layout). Prints "0 failure(s)" and returns 0 when everything holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime.h>

#include "../grammar_plan.h"

int launch_grammar_mask_budget(void* logits, int dtype, int B, int V, int64_t ld, const int* meta, const uint8_t* cls,
                               const uint16_t* tab, int tab_entries, const uint8_t* accept, int state_cap,
                               int n_classes_cap, int byte_cap, const int* stops, int* state, int rows,
                               const int* tok_off, int64_t n_off, const uint8_t* tok_bytes, int64_t n_bytes,
                               const int64_t* out, const int64_t* step, int max_steps, int out_ld, const int* budget,
                               int budget_rows, const uint16_t* c_acc, const uint16_t* c_pop, int need_states,
                               const uint8_t* all_live, int flag_states, hipStream_t stream);

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      ++failures;                                                     \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
    }                                                                 \
  } while (0)

static FILE* in = nullptr;
static long long next() {
  long long v = 0;
  if (std::fscanf(in, "%lld", &v) != 1) {
    std::printf("FAIL: the case file ended early\n");
    std::exit(2);
  }
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2 || (in = std::fopen(argv[1], "r")) == nullptr) {
    std::printf("usage: grammar_budget_check CASES\n");
    return 2;
  }
  const long long n_grammars = next();
  for (long long g = 0; g < n_grammars; ++g) {
    // the arrays sized exactly: an index one past any edge is a heap overflow the sanitizer reports
    gr::Table t;
    t.n_states = (int)next(), t.n_classes = 1;
    t.pop_obj = (int)next(), t.pop_arr = (int)next(), t.pop_empty = (int)next();
    t.trans = nullptr, t.cls = nullptr;     // need() reads neither
    std::vector<uint16_t> c_acc((size_t)t.n_states), c_pop((size_t)t.n_states);
    for (auto& v : c_acc) v = (uint16_t)next();
    for (auto& v : c_pop) v = (uint16_t)next();
    const gr::Need nd{c_acc.data(), c_pop.data()};
    const long long n_cases = next();
    for (long long i = 0; i < n_cases; ++i) {
      const int q = (int)next(), depth = (int)next();
      const uint32_t stack = (uint32_t)next();
      const int want = (int)next();
      const int got = gr::need(t, nd, q, depth, stack);
      if (got != want) {
        ++failures;
        std::printf("FAIL grammar %lld need(%d, %d, %u) = %d, the reference %d\n", g, q, depth, stack, got, want);
      }
    }
  }
  const long long n_rules = next();     // budget step need_after all_live need_cap -> r allows skippable
  for (long long i = 0; i < n_rules; ++i) {
    const int budget = (int)next();
    const long long step = next();
    const int need_after = (int)next(), all_live = (int)next(), cap = (int)next();
    const int r = (int)next(), allows = (int)next(), skip = (int)next();
    const int got = gr::remaining(budget, step);
    if (got != r || (int)gr::budget_allows(need_after, got) != allows ||
        (int)gr::walks_skippable(all_live != 0, cap, got) != skip) {
      ++failures;
      std::printf("FAIL rule %lld: r %d allows %d skip %d, expected %d %d %d\n", i, got,
                  (int)gr::budget_allows(need_after, got), (int)gr::walks_skippable(all_live != 0, cap, got), r, allows, skip);
    }
  }
  const long long n_plans = next();
  for (long long i = 0; i < n_plans; ++i) {
    long long a[18];
    for (auto& v : a) v = next();
    const int rc = (int)next(), chunks = (int)next();
    const gr::MaskPlan pl = gr::plan_grammar_budget((int)a[0], (int)a[1], a[2], (int)a[3], (int)a[4], (int)a[5], (int)a[6],
                                                    (int)a[7], a[8], a[9], (int)a[10], a[11] != 0, a[12] != 0, (int)a[13],
                                                    (int)a[14], (int)a[15], (int)a[16], (int)a[17]);
    if (pl.rc != rc || pl.chunks != chunks) {
      ++failures;
      std::printf("FAIL plan %lld: rc %d chunks %d, expected rc %d chunks %d\n", i, pl.rc, pl.chunks, rc, chunks);
    }
    if (rc != 0) {     // the launcher returns the plan's refusal before it touches a pointer or calls HIP
      int64_t dummy = 0;
      CHECK(launch_grammar_mask_budget(nullptr, (int)a[3], (int)a[0], (int)a[1], a[2], nullptr, nullptr, nullptr, (int)a[4],
                                       nullptr, (int)a[5], (int)a[6], (int)a[7], nullptr, nullptr, (int)a[10], nullptr, a[8],
                                       nullptr, a[9], a[11] ? &dummy : nullptr, a[12] ? &dummy : nullptr, (int)a[13],
                                       (int)a[14], nullptr, (int)a[17], nullptr, nullptr, (int)a[15], nullptr, (int)a[16],
                                       nullptr) == rc);
    }
  }
  // a batch of no rows is no launch; a shape in order with a null operand is refused, not launched
  CHECK(launch_grammar_mask_budget(nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, 0, 0, nullptr, nullptr, 0,
                                   nullptr, 0, nullptr, 0, nullptr, nullptr, 0, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, 0,
                                   nullptr) == 0);
  CHECK(launch_grammar_mask_budget(nullptr, 0, 3, 128256, 128256, nullptr, nullptr, nullptr, gr::MAX_TABLE, nullptr,
                                   gr::MAX_STATES, gr::MAX_CLASSES, gr::TOKEN_BYTE_CAP, nullptr, nullptr, 3, nullptr, 128257,
                                   nullptr, 16, nullptr, nullptr, 0, 0, nullptr, 3, nullptr, nullptr, gr::MAX_STATES, nullptr,
                                   gr::MAX_STATES, nullptr) == -11);
  CHECK(gr::NEED_INF > (gr::MAX_DEPTH + 1) * (int)gr::NEED_INF16 && gr::BUDGET_FREE - 2 < gr::NEED_INF);
  CHECK(!gr::budget_allows(gr::NEED_INF, gr::BUDGET_FREE) && gr::budget_allows(0, 2) && !gr::budget_allows(0, 1));
  std::fclose(in);
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
