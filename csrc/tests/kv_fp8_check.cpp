// The FP8 K/V cache's host-visible code, built with AddressSanitizer + UndefinedBehaviorSanitizer
// on the HOST code only and run without a GPU (tests/test_kv_fp8_host_check.py):
//   - the scalar rule of kv_fp8_core.h (the copy every cache writer runs) against a case file
//     written from ops/reference.py: every finite bf16 input x three inverse scales, byte for byte,
//     and the value of each of the 256 codes;
//   - the fp8 block layouts of common.h (kc8_elem / vc8_elem) are bijections on a block for
//     D = 128, and kc8_chunk / vc8_chunk name the same bytes;
//   - plan_paged_decode with an fp8 cache: D = 64 refused, lm = 7 falls back, both loop forms
//     reachable, and the bf16 answers (pinned field by field for the tuples of host_check.cpp) unchanged;
//   - every fp8 launcher rejects bad arguments BEFORE any HIP call.
// Case file (whitespace-separated integers): the number of inverse scales; per inverse scale its
// fp32 bits, then the expected code of every finite bf16 bit pattern in ascending order of the
// pattern; then for each of the 256 codes the fp32 bits of its value (-1: NaN).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "attn_plan.h"
#include "kv_fp8_core.h"

int launch_rope_cache_fp8(void* q_out, const void* qkv, const int64_t* positions, const float* cos_sin,
                          void* k_cache, void* v_cache, const int64_t* slots, int T, int Hq, int Hkv, int D, int BS,
                          int64_t qkv_stride, bool rope, float k_scale, float v_scale, hipStream_t stream);
int launch_paged_decode_fp8(void* out, const void* q, const void* k_cache, const void* v_cache,
                            const int* block_tables, const int* ctx_lens, float* part_o, float* part_ml,
                            int* counters, int B, int Hq, int Hkv, int D, int max_blocks, float scale, int num_splits,
                            const int* groups, int slot_stride, hipStream_t stream, const int* plan, int plan_stride,
                            float k_scale, float v_scale);
int launch_prefill_fp8(void* out, const void* q, const void* k_cache, const void* v_cache, const int* block_tables,
                       const int* cu_q, const int* start_pos, const int* tile_map, int n_tiles, int map_stride,
                       const int* cmap, int n_split, float* part_o, float* part_ml, int Hq, int Hkv, int D,
                       int max_blocks, float scale, float k_scale, float v_scale, hipStream_t stream);
int launch_skinny_gemm_rope_kv8(int wt, void* q_out, const void* x, const void* W, const void* wscale, int M, int K,
                                int pro, float eps, const int64_t* positions, const float* cos_sin, void* k_cache,
                                void* v_cache, const int64_t* slots, int Hq, int Hkv, int D, int BS, const void* x2,
                                void* xo, hipStream_t stream, int* split_ws, int64_t split_ws_ints, int split_mode,
                                const float* bias, float k_scale, float v_scale);

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static float bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }

static long check_rule(std::FILE* f) {
  long n_inv = 0, checked = 0;
  if (std::fscanf(f, "%ld", &n_inv) != 1) return -1;
  for (long s = 0; s < n_inv; ++s) {
    long inv_bits = 0;
    if (std::fscanf(f, "%ld", &inv_bits) != 1) return -1;
    const float inv = bits_f32((uint32_t)inv_bits);
    int bad = 0;
    unsigned prev = 0;
    bool first = true;
    // ascending bit patterns: 0x0000..0x7f7f are +0 .. +max, 0x8000..0xff7f are -0 .. -max
    for (uint32_t p = 0; p < 65536; ++p) {
      if (((p >> 7) & 0xffu) == 0xffu) continue;   // inf / NaN patterns are not in the file
      long want = 0;
      if (std::fscanf(f, "%ld", &want) != 1) return -1;
      const unsigned got = kv8::code(bits_f32(p << 16), inv);
      if (got != (unsigned)want && bad++ < 5)
        std::fprintf(stderr, "FAIL code: bf16 %04x inv %08lx: got %02x want %02lx\n", p, inv_bits, got, want);
      // monotone within each sign: the magnitude code never decreases with the magnitude
      if (p == 0x8000u) first = true;
      if (!first && (got & 0x7fu) < (prev & 0x7fu)) ++bad;
      prev = got, first = false;
      ++checked;
    }
    failures += bad;
  }
  for (unsigned c = 0; c < 256; ++c) {
    long want = 0;
    if (std::fscanf(f, "%ld", &want) != 1) return -1;
    const float v = kv8::e4m3_value(c);
    if (want < 0)
      EXPECT(v != v);
    else
      EXPECT(kv8::f32_bits(v) == (uint32_t)want);
    EXPECT(want < 0 || kv8::f32_bits(kv8::value(c, 1.f)) == (uint32_t)want);
  }
  return checked;
}

static void check_specials() {
  const float inf = INFINITY, nan = NAN;
  EXPECT(kv8::code(inf, 1.f) == 0x7eu && kv8::code(-inf, 1.f) == 0xfeu);       // saturate at +-448
  EXPECT(kv8::code(inf, 0.25f) == 0x7eu && kv8::code(1.0e30f, 1.f) == 0x7eu);
  EXPECT(kv8::code(nan, 1.f) == kv8::NAN_CODE && kv8::code(-nan, 0.25f) == kv8::NAN_CODE);
  EXPECT(kv8::code(448.f, 1.f) == 0x7eu && kv8::code(464.f, 1.f) == 0x7eu && kv8::code(1792.f, 0.25f) == 0x7eu);
  EXPECT(kv8::code(0.f, 1.f) == 0u && kv8::code(-0.f, 1.f) == 0x80u);
  EXPECT(kv8::e4m3_value(0) == 0.f && !std::signbit(kv8::e4m3_value(0)));       // zero bytes: a finite +0
  // ties to even: 17 is halfway between 16 (mantissa 000) and 18 (001); 19 between 18 and 20 (010)
  EXPECT(kv8::e4m3_value(kv8::code(17.f, 1.f)) == 16.f && kv8::e4m3_value(kv8::code(19.f, 1.f)) == 20.f);
  EXPECT(kv8::e4m3_value(kv8::code(-17.f, 1.f)) == -16.f);
  // below the smallest normal: multiples of 2^-9; 2^-10 is halfway between 0 and 2^-9 -> 0 (even)
  EXPECT(kv8::code(0.0009765625f, 1.f) == 0u && kv8::code(0.0029296875f, 1.f) == 2u);   // 1.5 * 2^-9 -> 2 * 2^-9
}

static void check_layouts() {
  constexpr int BS = 32, D = 128;
  std::vector<int> kseen(BS * D, 0), vseen(BS * D, 0);
  for (int key = 0; key < BS; ++key)
    for (int d = 0; d < D; ++d) {
      const int ko = rt::kc8_elem(BS, key, d), vo = rt::vc8_elem(BS, key, d);
      EXPECT(ko >= 0 && ko < BS * D && vo >= 0 && vo < BS * D);
      if (ko >= 0 && ko < BS * D) ++kseen[ko];
      if (vo >= 0 && vo < BS * D) ++vseen[vo];
    }
  int bad = 0;
  for (int i = 0; i < BS * D; ++i) bad += (kseen[i] != 1) + (vseen[i] != 1);
  EXPECT(bad == 0);
  // the chunk helpers name the same bytes: 16-B chunk w of a block
  for (int w = 0; w < BS * D / 16; ++w) {
    int key, c, d0, g;
    rt::kc8_chunk(w, BS, key, c);
    EXPECT(rt::kc8_elem(BS, key, 16 * c) == 16 * w && rt::kc8_elem(BS, key, 16 * c + 15) == 16 * w + 15);
    rt::vc8_chunk(w, d0, g);
    EXPECT(rt::vc8_elem(BS, 8 * g, d0) == 16 * w && rt::vc8_elem(BS, 8 * g + 7, d0) == 16 * w + 7);
    EXPECT(rt::vc8_elem(BS, 8 * g, d0 + 16) == 16 * w + 8 && rt::vc8_elem(BS, 8 * g + 7, d0 + 16) == 16 * w + 15);
  }
  // a decode K load instruction (16 rows r x 4 lane groups g x 16 B) covers whole 128-B lines
  for (int h = 0; h < 2; ++h)
    for (int c = 0; c < D / 64; ++c) {
      std::vector<int> line(BS * D / 128, 0);
      for (int r = 0; r < 16; ++r)
        for (int g = 0; g < 4; ++g)
          for (int j = 0; j < 16; ++j) ++line[rt::kc8_elem(BS, 8 * (r >> 2) + (r & 3) + 4 * h, 64 * c + 16 * g + j) / 128];
      for (int v : line) EXPECT(v == 0 || v == 128);
    }
}

static bool same_plan(const attn::AttnPlan& a, const attn::AttnPlan& b) {
  return a.rc == b.rc && a.splits == b.splits && a.gx == b.gx && a.gy == b.gy && a.block == b.block && a.GM == b.GM &&
         a.pp == b.pp && a.lm == b.lm && a.ext_combine == b.ext_combine && a.deferred == b.deferred &&
         a.combine == b.combine && a.nmax == b.nmax && a.nsl == b.nsl && a.spl == b.spl && a.cgx == b.cgx &&
         a.cgy == b.cgy && a.cblock == b.cblock;
}

static void check_plans() {
  using namespace attn;
  const AttnKnobs kn;
  // (B, Hq, Hkv, D, splits, grouped, stride, defer, has_plan, plan_stride): the tuples of host_check.cpp
  struct T { int B, Hq, Hkv, D, splits; bool grouped; int stride; bool defer, has_plan; int plan_stride; };
  const T tuples[] = {
      {3, 32, 8, 128, 10, true, 40, false, false, 0}, {3, 4, 1, 128, 64, true, 256, false, false, 0},
      {6, 32, 8, 128, 8, false, 0, false, false, 0},  {6, 32, 8, 128, 1, false, 0, false, false, 0},
      {3, 32, 8, 128, 1, true, 4, false, false, 0},   {2, 12, 12, 64, 3, false, 0, false, false, 0},
      {2, 20, 4, 128, 3, false, 0, false, false, 0},  {2, 28, 4, 128, 3, false, 0, false, false, 0},
      {2, 64, 8, 128, 3, false, 0, false, false, 0},  {2, 36, 4, 128, 3, false, 0, false, false, 0},
      {2, 64, 4, 128, 3, false, 0, false, false, 0},  {2, 12, 12, 64, 3, true, 48, false, false, 0},
      {0, 30, 8, 100, 65, true, 2, false, true, 8},   {2, 30, 8, 100, 65, true, 2, false, true, 8},
      {2, 64, 2, 100, 65, true, 2, false, true, 8},   {2, 32, 8, 128, 0, false, 0, false, false, 0},
      {2, 32, 8, 128, -5, true, 1, false, false, 0},  {2, 32, 8, 100, 65, true, 2, false, true, 8},
      {2, 32, 8, 128, 64, false, 0, false, false, 0}, {2, 32, 8, 100, 4, true, 2, false, true, 8},
      {2, 32, 8, 100, 4, false, 2, false, false, 8},  {2, 32, 8, 100, 4, true, 4, false, true, 8},
      {2, 32, 8, 100, 4, true, 4, false, true, 9},    {2, 32, 8, 128, 4, true, 4, false, true, 9},
      {2, 32, 8, 96, 4, false, 0, false, false, 0},   {2, 32, 8, 256, 4, false, 0, false, false, 0},
      {3, 32, 8, 128, 10, true, 40, true, false, 0},  {2, 12, 12, 64, 3, false, 0, true, false, 0},
      {3, 32, 8, 128, 1, true, 4, true, false, 0},    {2, 16, 4, 128, 3, false, 0, false, false, 0},
      {2, 6, 3, 128, 3, false, 0, false, false, 0},
  };
  for (const T& t : tuples) {
    const AttnPlan old = plan_paged_decode(t.B, t.Hq, t.Hkv, t.D, t.splits, t.grouped, t.stride, t.has_plan,
                                           t.plan_stride, t.defer, kn);
    AttnPlan f8 = plan_paged_decode(t.B, t.Hq, t.Hkv, t.D, t.splits, t.grouped, t.stride, t.has_plan, t.plan_stride,
                                    t.defer, kn, true);
    if (t.B == 0) {
      EXPECT(f8.rc == 0 && f8.gx == 0);
    } else if (old.rc != 0) {
      EXPECT(f8.rc == old.rc);    // earlier refusals keep their code and their order
    } else if (t.D != 128) {
      EXPECT(f8.rc == -7);        // fp8 caches: D = 128 only
    } else {
      // the same launch, except that the combine is never left to the caller
      EXPECT(f8.rc == 0 && !f8.deferred && f8.gx == old.gx && f8.gy == old.gy && f8.GM == old.GM && f8.pp == old.pp &&
             f8.lm == old.lm && f8.ext_combine == old.ext_combine);
      if (!old.deferred) EXPECT(same_plan(f8, old));
      if (old.deferred) EXPECT(f8.combine && f8.cgx == t.B * t.Hq && f8.cgy == 4);
    }
  }
  // The bf16 answers (no fp8 argument) are the ones host_check.cpp pins, worked out by hand from the
  // launcher's rules before the plan took an fp8 argument: every field of three of its tuples, its
  // return codes, and the D = 64 plan, repeated here so that this file fails too if they move.
  const auto pinned = [](const AttnPlan& p, int gx, int gy, int GM, bool pp, int lm, bool ext, bool deferred,
                         bool combine, int nmax, int nsl, int spl, int cgx, int cgy) {
    return p.rc == 0 && p.gx == gx && p.gy == gy && p.splits == gy && p.block == 512 && p.GM == GM && p.pp == pp &&
           p.lm == lm && p.ext_combine == ext && p.deferred == deferred && p.combine == combine && p.nmax == nmax &&
           p.nsl == nsl && p.spl == spl && p.cgx == cgx && p.cgy == cgy && p.cblock == 8 * nsl;
  };
  EXPECT(pinned(plan_paged_decode(3, 32, 8, 128, 10, true, 40, false, 0, false, kn), 24, 10, 16, true, 3, true, false,
                true, 40, 24, 2, 96, 4));
  EXPECT(pinned(plan_paged_decode(3, 4, 1, 128, 64, true, 256, false, 0, false, kn), 3, 64, 16, false, 3, true, false,
                true, 256, 32, 8, 12, 4));
  EXPECT(pinned(plan_paged_decode(6, 32, 8, 128, 8, false, 0, false, 0, false, kn), 48, 8, 4, true, 3, true, false,
                true, 8, 8, 1, 192, 4));
  EXPECT(pinned(plan_paged_decode(2, 12, 12, 64, 3, false, 0, false, 0, false, kn), 24, 3, 4, true, 3, true, false,
                true, 3, 8, 1, 24, 2));
  EXPECT(pinned(plan_paged_decode(3, 32, 8, 128, 10, true, 40, false, 0, true, kn), 24, 10, 16, true, 3, true, true,
                false, 0, 0, 0, 0, 0));                                   // deferred to the caller
  EXPECT(plan_paged_decode(2, 30, 8, 100, 65, true, 2, true, 8, false, kn).rc == -1);
  EXPECT(plan_paged_decode(2, 32, 8, 100, 65, true, 2, true, 8, false, kn).rc == -3);
  EXPECT(plan_paged_decode(2, 32, 8, 100, 4, true, 2, true, 8, false, kn).rc == -4);
  EXPECT(plan_paged_decode(2, 32, 8, 100, 4, true, 4, true, 8, false, kn).rc == -5);
  EXPECT(plan_paged_decode(2, 32, 8, 96, 4, false, 0, false, 0, false, kn).rc == -2);
  // the contract's names are the same rule
  EXPECT(kv_fp8_code(19.f, 1.f) == kv8::code(19.f, 1.f) && kv_fp8_code(-3.f, 0.25f) == kv8::code(-3.f, 0.25f));
  EXPECT(kv_fp8_value(0x5au, 2.f) == 40.f);
  // both loop forms are reachable with an fp8 cache: ping-pong at Hkv >= 4, the copy loop below
  EXPECT(plan_paged_decode(3, 32, 8, 128, 10, true, 40, false, 0, false, kn, true).pp);
  EXPECT(!plan_paged_decode(3, 8, 1, 128, 64, true, 256, false, 0, false, kn, true).pp);
  // GM 4 / 8 / 16
  EXPECT(plan_paged_decode(2, 32, 8, 128, 3, false, 0, false, 0, false, kn, true).GM == 4);
  EXPECT(plan_paged_decode(2, 8, 1, 128, 3, false, 0, false, 0, false, kn, true).GM == 8);
  EXPECT(plan_paged_decode(2, 8, 1, 128, 3, true, 6, false, 0, false, kn, true).GM == 16);
  // RT_ATTN_LM=7 (LDS-DMA staged loop) does not exist for fp8: its two nt bits remain
  AttnKnobs k7;
  k7.lm = 7;
  EXPECT(plan_paged_decode(3, 32, 8, 128, 10, true, 40, false, 0, false, k7).lm == 7);
  EXPECT(plan_paged_decode(3, 32, 8, 128, 10, true, 40, false, 0, false, k7, true).lm == 3);
  k7.lm = 5;
  EXPECT(plan_paged_decode(3, 32, 8, 128, 10, true, 40, false, 0, false, k7, true).lm == 1);
  EXPECT(plan_paged_decode(2, 12, 12, 64, 3, false, 0, false, 0, false, k7, true).rc == -7);
}

static void check_launchers() {
  void* const n = nullptr;
  // decode: plan refusals, then D = 64 (-7), scales (-8); B = 0 is an empty launch
  EXPECT(launch_paged_decode_fp8(n, n, n, n, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 12, 12, 64, 4, 1.f, 3,
                                 nullptr, 0, nullptr, nullptr, 0, 1.f, 1.f) == -7);
  EXPECT(launch_paged_decode_fp8(n, n, n, n, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 30, 8, 128, 4, 1.f, 3,
                                 nullptr, 0, nullptr, nullptr, 0, 1.f, 1.f) == -1);
  EXPECT(launch_paged_decode_fp8(n, n, n, n, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 32, 8, 128, 4, 1.f, 65,
                                 nullptr, 0, nullptr, nullptr, 0, 1.f, 1.f) == -3);
  EXPECT(launch_paged_decode_fp8(n, n, n, n, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 32, 8, 96, 4, 1.f, 3,
                                 nullptr, 0, nullptr, nullptr, 0, 1.f, 1.f) == -2);
  const float bad[] = {0.f, -1.f, INFINITY, NAN};
  for (float s : bad) {
    EXPECT(launch_paged_decode_fp8(n, n, n, n, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 32, 8, 128, 4, 1.f, 3,
                                   nullptr, 0, nullptr, nullptr, 0, s, 1.f) == -8);
    EXPECT(launch_paged_decode_fp8(n, n, n, n, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 32, 8, 128, 4, 1.f, 3,
                                   nullptr, 0, nullptr, nullptr, 0, 1.f, s) == -8);
    EXPECT(launch_rope_cache_fp8(n, n, nullptr, nullptr, n, n, nullptr, 4, 4, 1, 128, 32, 768, false, s, 1.f,
                                 nullptr) == -1);
    EXPECT(launch_rope_cache_fp8(n, n, nullptr, nullptr, n, n, nullptr, 4, 4, 1, 128, 32, 768, false, 1.f, s,
                                 nullptr) == -1);
    EXPECT(launch_prefill_fp8(n, n, n, n, nullptr, nullptr, nullptr, nullptr, 1, 2, nullptr, 0, nullptr, nullptr, 4, 1,
                              128, 4, 1.f, s, 1.f, nullptr) == -4);
    EXPECT(launch_prefill_fp8(n, n, n, n, nullptr, nullptr, nullptr, nullptr, 1, 2, nullptr, 0, nullptr, nullptr, 4, 1,
                              128, 4, 1.f, 1.f, s, nullptr) == -4);
    EXPECT(launch_skinny_gemm_rope_kv8(0, n, n, n, nullptr, 1, 64, 0, 1e-5f, nullptr, nullptr, n, n, nullptr, 2, 1, 128,
                                       32, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, s, 1.f) == -7);
    EXPECT(launch_skinny_gemm_rope_kv8(0, n, n, n, nullptr, 1, 64, 0, 1e-5f, nullptr, nullptr, n, n, nullptr, 2, 1, 128,
                                       32, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 1.f, s) == -7);
  }
  EXPECT(launch_paged_decode_fp8(n, n, n, n, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 32, 8, 128, 4, 1.f, 3,
                                 nullptr, 0, nullptr, nullptr, 0, 1.f, 1.f) == 0);
  // writer: head dims / block sizes outside the fp8 layouts, a missing RoPE table, null operands
  EXPECT(launch_rope_cache_fp8(n, n, nullptr, nullptr, n, n, nullptr, 4, 4, 1, 96, 32, 576, false, 1.f, 1.f, nullptr) == -1);
  EXPECT(launch_rope_cache_fp8(n, n, nullptr, nullptr, n, n, nullptr, 4, 4, 1, 128, 4, 768, false, 1.f, 1.f, nullptr) == -1);
  EXPECT(launch_rope_cache_fp8(n, n, nullptr, nullptr, n, n, nullptr, 4, 4, 1, 128, 32, 768, true, 1.f, 1.f, nullptr) == -1);
  EXPECT(launch_rope_cache_fp8(n, n, nullptr, nullptr, n, n, nullptr, 4, 4, 1, 128, 32, 768, false, 1.f, 1.f, nullptr) == -1);
  EXPECT(launch_rope_cache_fp8(n, n, nullptr, nullptr, n, n, nullptr, 0, 4, 1, 128, 32, 768, false, 1.f, 1.f, nullptr) == 0);
  // prefill: the 16x16 kernel's shapes are refused (D != 128, G > 8, a ragged head ratio), bad map strides
  EXPECT(launch_prefill_fp8(n, n, n, n, nullptr, nullptr, nullptr, nullptr, 1, 2, nullptr, 0, nullptr, nullptr, 12, 12,
                            64, 4, 1.f, 1.f, 1.f, nullptr) == -1);
  EXPECT(launch_prefill_fp8(n, n, n, n, nullptr, nullptr, nullptr, nullptr, 1, 2, nullptr, 0, nullptr, nullptr, 16, 1,
                            128, 4, 1.f, 1.f, 1.f, nullptr) == -1);
  EXPECT(launch_prefill_fp8(n, n, n, n, nullptr, nullptr, nullptr, nullptr, 1, 2, nullptr, 0, nullptr, nullptr, 30, 8,
                            128, 4, 1.f, 1.f, 1.f, nullptr) == -1);
  EXPECT(launch_prefill_fp8(n, n, n, n, nullptr, nullptr, nullptr, nullptr, 1, 3, nullptr, 0, nullptr, nullptr, 4, 1,
                            128, 4, 1.f, 1.f, 1.f, nullptr) == -2);
  const int cmap[4] = {0, 0, 0, 2};
  EXPECT(launch_prefill_fp8(n, n, n, n, nullptr, nullptr, nullptr, nullptr, 1, 5, cmap, 1, nullptr, nullptr, 4, 1, 128,
                            4, 1.f, 1.f, 1.f, nullptr) == -3);
  EXPECT(launch_prefill_fp8(n, n, n, n, nullptr, nullptr, nullptr, nullptr, 0, 2, nullptr, 0, nullptr, nullptr, 4, 1,
                            128, 4, 1.f, 1.f, 1.f, nullptr) == 0);
  // GEMM epilogue: head dim / block size outside the fp8 layouts, unknown weight type, width mismatch
  EXPECT(launch_skinny_gemm_rope_kv8(0, n, n, n, nullptr, 1, 64, 0, 1e-5f, nullptr, nullptr, n, n, nullptr, 2, 1, 96, 32,
                                     nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 1.f, 1.f) == -7);
  EXPECT(launch_skinny_gemm_rope_kv8(0, n, n, n, nullptr, 1, 64, 0, 1e-5f, nullptr, nullptr, n, n, nullptr, 2, 1, 128, 4,
                                     nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 1.f, 1.f) == -7);
  EXPECT(launch_skinny_gemm_rope_kv8(3, n, n, n, nullptr, 1, 64, 0, 1e-5f, nullptr, nullptr, n, n, nullptr, 2, 1, 128, 32,
                                     nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 1.f, 1.f) == -1);
  EXPECT(launch_skinny_gemm_rope_kv8(0, n, n, n, nullptr, 17, 64, 2, 1e-5f, nullptr, nullptr, n, n, nullptr, 2, 1, 128,
                                     32, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 1.f, 1.f) == -5);
  EXPECT(launch_skinny_gemm_rope_kv8(1, n, n, n, nullptr, 1, 64, 0, 1e-5f, nullptr, nullptr, n, n, nullptr, 2, 1, 128, 32,
                                     nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 1.f, 1.f) == -1);   // no wscale
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: kv_fp8_check <case file>\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const long codes = check_rule(f);
  std::fclose(f);
  EXPECT(codes > 0);
  check_specials();
  check_layouts();
  check_plans();
  check_launchers();
  std::printf("%ld codes, 256 values, %d failure(s)\n", codes, failures);
  return failures == 0 ? 0 : 1;
}
