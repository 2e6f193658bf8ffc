// The QK-norm kernel's host-visible code (qk_norm_plan.h and the launcher of qk_norm_rope.hip), built
// with AddressSanitizer + UndefinedBehaviorSanitizer on the HOST code only and run without a GPU
// (tests/test_qk_norm_host_check.py):
//   - the plan's grid for every shape of a case file (whitespace-separated integers, one
//     "T Hq Hkv D grid" record per case, written from ops/oracle64.py's shape lists);
//   - every refusal code of the plan;
//   - the launcher returns the plan's code BEFORE any HIP call on each refusal, and 0 for T = 0.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "qk_norm_plan.h"

int launch_qk_norm_rope(void* q_out, const void* qkv, const int64_t* positions, const float* cos_sin,
                        const void* q_gamma, const void* k_gamma, float eps, void* k_cache, void* v_cache,
                        const int64_t* slots, int T, int Hq, int Hkv, int D, int BS, int64_t qkv_stride, bool rope,
                        bool kv8, float k_scale, float v_scale, hipStream_t stream);

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

// the launcher with every operand present (never dereferenced on the host) but the ones a case names
static int launch(int T, int Hq, int Hkv, int D, int BS, bool rope, bool kv8, float ks, float vs, float eps,
                  bool with_table = true, bool with_gamma = true) {
  static int64_t word[2] = {0, 0};
  void* p = word;
  const int64_t* ip = word;
  return launch_qk_norm_rope(p, p, ip, with_table ? reinterpret_cast<const float*>(word) : nullptr,
                             with_gamma ? p : nullptr, p, eps, p, p, ip, T, Hq, Hkv, D, BS,
                             (int64_t)(Hq + 2 * Hkv) * D, rope, kv8, ks, vs, nullptr);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: qk_norm_check CASES\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  long grids = 0, T, Hq, Hkv, D, grid;
  while (std::fscanf(f, "%ld %ld %ld %ld %ld", &T, &Hq, &Hkv, &D, &grid) == 5) {
    for (int kv8 = 0; kv8 < 2; ++kv8) {
      if (kv8 && D % 64) continue;
      const int g = qkn::plan(T, (int)Hq, (int)Hkv, (int)D, 32, kv8 != 0, 1.f, 0.37f, 1e-6f);
      EXPECT(g == (int)grid);
      EXPECT((int64_t)g * qkn::WAVES >= T * (Hq + 2 * Hkv) && (int64_t)(g - 1) * qkn::WAVES < T * (Hq + 2 * Hkv));
    }
    ++grids;
  }
  std::fclose(f);
  EXPECT(qkn::WAVES == 4 && qkn::THREADS == 256);

  const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
  // head_dim: 64 and 128 only
  for (int D : {0, 32, 96, 192, 256, -128}) {
    EXPECT(qkn::plan(3, 4, 1, D, 32, false, 1.f, 1.f, 1e-6f) == -1);
    EXPECT(launch(3, 4, 1, D, 32, true, false, 1.f, 1.f, 1e-6f) == -1);
  }
  EXPECT(qkn::plan(3, 4, 1, 64, 32, false, 1.f, 1.f, 1e-6f) == 5 && qkn::plan(3, 4, 1, 128, 32, false, 1.f, 1.f, 0.f) == 5);
  // fp8 cache: block_size % 8 (D % 64 holds for both head dims the kernel takes)
  EXPECT(qkn::plan(3, 4, 1, 128, 12, true, 1.f, 1.f, 1e-6f) == -1);
  EXPECT(qkn::plan(3, 4, 1, 128, 12, false, 1.f, 1.f, 1e-6f) == 5);
  EXPECT(launch(3, 4, 1, 128, 12, true, true, 1.f, 1.f, 1e-6f) == -1);
  EXPECT(qkn::plan(3, 4, 1, 128, 0, false, 1.f, 1.f, 1e-6f) == -1);
  EXPECT(qkn::plan(3, 0, 1, 128, 32, false, 1.f, 1.f, 1e-6f) == -1 && qkn::plan(3, 4, 0, 128, 32, false, 1.f, 1.f, 1e-6f) == -1);
  EXPECT(qkn::plan(-1, 4, 1, 128, 32, false, 1.f, 1.f, 1e-6f) == -1);
  // scales: finite, > 0, <= 3e38
  for (float s : {0.f, -1.f, inf, -inf, nan, 3.2e38f}) {
    EXPECT(qkn::plan(3, 4, 1, 128, 32, true, s, 1.f, 1e-6f) == -1);
    EXPECT(qkn::plan(3, 4, 1, 128, 32, true, 1.f, s, 1e-6f) == -1);
    EXPECT(launch(3, 4, 1, 128, 32, true, true, s, 1.f, 1e-6f) == -1);
    EXPECT(launch(3, 4, 1, 128, 32, false, true, 1.f, s, 1e-6f) == -1);
  }
  EXPECT(qkn::plan(3, 4, 1, 128, 32, true, 3.0e38f, 1e-30f, 1e-6f) == 5);
  // eps: finite, >= 0
  for (float e : {-1e-6f, inf, -inf, nan}) {
    EXPECT(qkn::plan(3, 4, 1, 128, 32, false, 1.f, 1.f, e) == -1);
    EXPECT(launch(3, 4, 1, 128, 32, true, false, 1.f, 1.f, e) == -1);
  }
  // more waves than a 32-bit index holds: -2 (2^31 - 1 itself is taken)
  EXPECT(qkn::plan(44739243, 32, 8, 128, 32, false, 1.f, 1.f, 1e-6f) == -2);      // 48 T = 2^31 + 16
  EXPECT(qkn::plan(44739242, 32, 8, 128, 32, false, 1.f, 1.f, 1e-6f) == 536870904);   // 48 T = 2^31 - 32
  EXPECT(qkn::plan(2147483647, 1, 0 + 1, 64, 32, false, 1.f, 1.f, 1e-6f) == -2);
  EXPECT(launch(44739243, 32, 8, 128, 32, true, false, 1.f, 1.f, 1e-6f) == -2);
  // T == 0: a zero grid, no launch, whatever the operands
  EXPECT(qkn::plan(0, 32, 8, 128, 32, true, 1.f, 1.f, 1e-6f) == 0);
  EXPECT(qkn::plan(0, 32, 8, 128, 32, true, 1.f, 1.f, 1e-6f, false) == 0);
  EXPECT(launch(0, 32, 8, 128, 32, true, true, 1.f, 1.f, 1e-6f) == 0);
  EXPECT(launch(0, 32, 8, 128, 32, true, false, 1.f, 1.f, 1e-6f, false, false) == 0);
  // a missing operand: the table of a rotating launch, a gamma
  EXPECT(qkn::plan(3, 4, 1, 128, 32, false, 1.f, 1.f, 1e-6f, false) == -1);
  EXPECT(launch(3, 4, 1, 128, 32, true, false, 1.f, 1.f, 1e-6f, false) == -1);
  EXPECT(launch(3, 4, 1, 128, 32, false, false, 1.f, 1.f, 1e-6f, true, false) == -1);

  std::printf("%ld grids, %d failure(s)\n", grids, failures);
  return failures ? 1 : 0;
}
