// Host check of the grammar mask's host-visible parts, without a GPU: the walk of csrc/grammar_core.h
// (the copy the kernel runs) against cases the Python reference wrote, the refusals of
// plan_grammar_mask (csrc/grammar_plan.h), and the launcher's argument validation, which must reject
// before any HIP call. Reads one file of whitespace-separated integers (tests/test_grammar_host_check.py
// writes it and documents the layout). Prints "0 failure(s)" and returns 0 when everything holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime.h>

#include "../grammar_plan.h"

int launch_grammar_mask(void* logits, int dtype, int B, int V, int64_t ld, const int* meta, const uint8_t* cls,
                        const uint16_t* tab, int tab_entries, const uint8_t* accept, int state_cap, int n_classes_cap,
                        int byte_cap, const int* stops, int* state, int rows, const int* tok_off, int64_t n_off,
                        const uint8_t* tok_bytes, int64_t n_bytes, const int64_t* out, const int64_t* step,
                        int max_steps, int out_ld, hipStream_t stream);

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
    std::printf("usage: grammar_check CASES\n");
    return 2;
  }
  // the table, sized exactly: an index one past any edge is a heap overflow the sanitizer reports
  gr::Table t;
  t.n_states = (int)next(), t.n_classes = (int)next();
  t.pop_obj = (int)next(), t.pop_arr = (int)next(), t.pop_empty = (int)next();
  std::vector<uint8_t> cls(256);
  for (auto& c : cls) c = (uint8_t)next();
  std::vector<uint16_t> trans((size_t)t.n_states * t.n_classes);
  for (auto& e : trans) e = (uint16_t)next();
  t.cls = cls.data(), t.trans = trans.data();
  std::vector<int> stops((size_t)next());
  for (auto& s : stops) s = (int)next();
  const int V = (int)next();
  std::vector<int> off((size_t)V + 1);
  for (auto& o : off) o = (int)next();
  std::vector<uint8_t> bytes((size_t)next());
  for (auto& b : bytes) b = (uint8_t)next();

  const long long n_cases = next();
  for (long long i = 0; i < n_cases; ++i) {
    const int kind = (int)next();     // 0: walk over given bytes, 1: advance over a token id
    gr::State s;
    s.q = (int)next(), s.depth = (int)next(), s.stack = (uint32_t)next();
    bool alive = true;
    if (kind == 0) {
      std::vector<uint8_t> data((size_t)next());
      for (auto& b : data) b = (uint8_t)next();
      alive = gr::walk(t, s, data.data(), (int)data.size());
    } else {
      const long long tok = next();
      gr::advance(t, s, stops.data(), (int)stops.size(), off.data(), bytes.data(), (int64_t)bytes.size(), V, tok);
    }
    const int q = (int)next(), depth = (int)next();
    const uint32_t stack = (uint32_t)next();
    if (s.q != q || s.depth != depth || s.stack != stack || (kind == 0 && alive != (q >= 0 || q == gr::Q_FIN))) {
      ++failures;
      std::printf("FAIL case %lld (kind %d): got (%d, %d, %u), the reference (%d, %d, %u)\n", i, kind, s.q, s.depth,
                  s.stack, q, depth, stack);
    }
  }

  const long long n_plans = next();
  for (long long i = 0; i < n_plans; ++i) {
    long long a[15];
    for (auto& v : a) v = next();
    const int rc = (int)next(), chunks = (int)next();
    const gr::MaskPlan pl = gr::plan_grammar_mask((int)a[0], (int)a[1], a[2], (int)a[3], (int)a[4], (int)a[5], (int)a[6],
                                                  (int)a[7], a[8], a[9], (int)a[10], a[11] != 0, a[12] != 0, (int)a[13],
                                                  (int)a[14]);
    if (pl.rc != rc || (rc == 0 && pl.chunks != chunks)) {
      ++failures;
      std::printf("FAIL plan %lld: rc %d chunks %d, expected rc %d chunks %d\n", i, pl.rc, pl.chunks, rc, chunks);
    }
    // the launcher returns the plan's refusal before it touches a pointer or calls HIP
    if (rc != 0) {
      int64_t dummy = 0;
      CHECK(launch_grammar_mask(nullptr, (int)a[3], (int)a[0], (int)a[1], a[2], nullptr, nullptr, nullptr, (int)a[4],
                                nullptr, (int)a[5], (int)a[6], (int)a[7], nullptr, nullptr, (int)a[10], nullptr, a[8],
                                nullptr, a[9], a[11] ? &dummy : nullptr, a[12] ? &dummy : nullptr, (int)a[13],
                                (int)a[14], nullptr) == rc);
    }
  }
  // a batch of no rows is no launch; a shape in order with a null operand is refused, not launched
  CHECK(launch_grammar_mask(nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, 0, 0, nullptr, nullptr, 0,
                            nullptr, 0, nullptr, 0, nullptr, nullptr, 0, 0, nullptr) == 0);
  CHECK(launch_grammar_mask(nullptr, 0, 3, 128256, 128256, nullptr, nullptr, nullptr, gr::MAX_TABLE, nullptr,
                            gr::MAX_STATES, gr::MAX_CLASSES, gr::TOKEN_BYTE_CAP, nullptr, nullptr, 3, nullptr, 128257,
                            nullptr, 16, nullptr, nullptr, 0, 0, nullptr) == -11);
  CHECK(gr::LDS_ENTRIES % 8 == 0 && gr::LDS_ENTRIES * 2 <= 64 * 1024 && gr::MAX_TABLE % 8 == 0);
  CHECK(gr::MAX_STATES * 4 - 1 < gr::DEAD_ENTRY);     // every (q' << 2 | action) is distinct from the dead entry
  std::fclose(in);
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
