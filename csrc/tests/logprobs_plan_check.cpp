// Host check of csrc/logprobs_plan.h: the chunk count, the workspace size and every refusal of the
// logprob launcher, without a GPU (the header holds no device code). Prints "0 failure(s)" and
// returns 0 when every rule holds.
#include "../logprobs_plan.h"

#include <cstdio>

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      ++failures;                                                     \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
    }                                                                 \
  } while (0)

using namespace lpr;

// the eager form of a B-row batch with everything in order, one field changed by the caller
struct Case {
  int B = 3, V = 128256;
  int64_t ld = 128256;
  int dtype = 0, rec_cols = MAX_TOP, rec_ld = 3, rec_steps = 1;
  bool ids = true, out = false, step = false;
  int max_steps = 0, out_ld = 0;
  int64_t ws = workspace_words(3);
  LogprobPlan plan() const {
    return plan_logprobs(B, V, ld, dtype, rec_cols, rec_ld, rec_steps, ids, out, step, max_steps, out_ld, ws);
  }
};

int main() {
  CHECK(Case().plan().rc == 0 && Case().plan().nch == 32);     // Llama-3: 32 chunks
  {
    Case c;
    c.V = 152064, c.ld = 152064;
    CHECK(c.plan().rc == 0 && c.plan().nch == 38);              // Qwen2: 38
    c.V = c.ld = 1;
    CHECK(c.plan().nch == 1);
    c.V = c.ld = 4096;
    CHECK(c.plan().nch == 1);
    c.V = c.ld = 4097;
    CHECK(c.plan().nch == 2);
    c.V = c.ld = MAX_CHUNKS * CHUNK;
    CHECK(c.plan().rc == 0 && c.plan().nch == MAX_CHUNKS);
    c.V = c.ld = MAX_CHUNKS * CHUNK + 1;
    CHECK(c.plan().rc == -2);
  }
  CHECK(workspace_words(3) == 3 * 64 * 44 && workspace_words(0) == 0 && workspace_words(-1) == 0);
  CHECK(WS_KEY % 4 == 0 && WS_REC == 44 && WS_ID + MAX_TOP == WS_REC);
  {
    Case c;
    c.V = 0;
    CHECK(c.plan().rc == -1);
    c = Case();
    c.ld = c.V - 1;
    CHECK(c.plan().rc == -1);
    c = Case();
    c.ld = c.V + 8;
    CHECK(c.plan().rc == 0);
    c = Case();
    c.dtype = 2;
    CHECK(c.plan().rc == -3);
    c.dtype = 1;
    CHECK(c.plan().rc == 0);
    c = Case();
    c.rec_cols = MAX_TOP - 1;
    CHECK(c.plan().rc == -4);
    c = Case();
    c.out = true;                                               // out without step
    CHECK(c.plan().rc == -5);
    c = Case();
    c.step = true;                                              // step without out
    CHECK(c.plan().rc == -5);
    c = Case();
    c.ids = false;                                              // neither form
    CHECK(c.plan().rc == -5);
    c = Case();
    c.out = c.step = true, c.max_steps = 1, c.out_ld = 2;       // out narrower than the batch
    CHECK(c.plan().rc == -6);
    c.out_ld = 3;
    CHECK(c.plan().rc == 0);
    c.max_steps = 2;                                            // more steps than record rows
    CHECK(c.plan().rc == -7);
    c = Case();
    c.rec_ld = 2;
    CHECK(c.plan().rc == -7);
    c = Case();
    c.ws -= 1;
    CHECK(c.plan().rc == -8);
  }
  std::printf("%d failure(s)\n", failures);
  return failures != 0;
}
