// The MXFP4 path's host-visible code under AddressSanitizer + UndefinedBehaviorSanitizer, without a
// GPU (its own main; nothing is preloaded): the scalar rule of fp4_core.h — the copy the quantise /
// dequantise kernels run — against the cases ops/reference.py wrote, the lane-record map for
// WT_FP4, the launch plan, weight_shape_ok and the launchers' argument validation, which rejects
// before any HIP call. Build + run: tests/test_mxfp4_host_check.py (the case-file format is there).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "fp4_core.h"
#include "skinny_plan.h"

int launch_skinny_gemm_fp4(void* out, const void* x, const void* Wq, const uint8_t* scale, void* res, int M, int N,
                           int K, int ldo, float eps, int pro, int epi, const void* rope, hipStream_t stream);
int launch_skinny_gemm_rope_fp4(void* q_out, const void* x, const void* Wq, const uint8_t* scale, int M, int K,
                                int pro, float eps, const int64_t* positions, const float* cos_sin, void* k_cache,
                                void* v_cache, const int64_t* slots, int Hq, int Hkv, int D, int BS,
                                const float* bias, hipStream_t stream);
int launch_shuffle_weight_fp4(void* Wq, uint8_t* scale, const void* W, const void* gamma, int N, int K,
                              int rope_rows, int D, int swiglu, hipStream_t stream);
int launch_unshuffle_weight_fp4(void* W, const void* Wq, const uint8_t* scale, int N, int K, int rope_rows, int D,
                                int swiglu, hipStream_t stream);

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      if (failures < 50) std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static bool read_int(FILE* f, long long& v) { return std::fscanf(f, "%lld", &v) == 1; }

static float bf16_value(unsigned bits) { return fp4::bits_f32((uint32_t)bits << 16); }
static bool bf16_finite(unsigned bits) { return ((bits >> 7) & 0xffu) != 0xffu; }

// code of every finite bf16 bit pattern under each listed scale byte; value of every code
static long check_codes(FILE* f) {
  long long n_scales = 0;
  long checked = 0;
  EXPECT(read_int(f, n_scales) && n_scales > 0);
  for (long long i = 0; i < n_scales; ++i) {
    long long e = 0;
    EXPECT(read_int(f, e) && e >= fp4::SCALE_MIN && e <= fp4::SCALE_MAX);
    for (unsigned bits = 0; bits < 65536u; ++bits) {
      if (!bf16_finite(bits)) continue;
      long long want = -1;
      if (!read_int(f, want)) {
        EXPECT(!"case file truncated");
        return checked;
      }
      EXPECT((long long)fp4::code(bf16_value(bits), (unsigned)e) == want);
      ++checked;
    }
    for (unsigned c = 0; c < 16u; ++c) {   // value(code, e) as the bf16 bits the reference dequantises to
      long long want = -1;
      EXPECT(read_int(f, want));
      const uint32_t got = fp4::f32_bits(fp4::value(c, (unsigned)e));
      EXPECT((got & 0xffffu) == 0u && (long long)(got >> 16) == want);
    }
  }
  return checked;
}

// scale byte of amax values (fp32 bit patterns) across the exponent range
static long check_scales(FILE* f) {
  long long n = 0;
  EXPECT(read_int(f, n) && n > 0);
  for (long long i = 0; i < n; ++i) {
    long long bits = 0, want = 0;
    EXPECT(read_int(f, bits) && read_int(f, want));
    EXPECT((long long)fp4::scale_byte(fp4::bits_f32((uint32_t)bits)) == want);
  }
  EXPECT(fp4::scale_byte(0.f) == 2u);
  return (long)n;
}

// lane_record<WT_FP4> on an [N, K] weight: a bijection onto the records, and every lane at the
// place the layout states: record (t, s, h, l) holds row 16t + (l&15) + h*N/2 (ROPE rows
// pair-interleaved inside their head), k0 = 128s + 32(l>>4), at chunk / tile-major offset
static void check_layout(int N, int K, int rope_rows, int D, bool swiglu, int order) {
  using namespace skinny;
  const int ks = K / 128, T = swiglu ? N / 32 : N / 16, H = swiglu ? 2 : 1;
  const int64_t total = lane_records<WT_FP4>(N, K);
  EXPECT(total == (int64_t)N * K / 32);
  // records per chunk: the bf16 order's k range, 2^(order-1) 32-deep steps, in 128-deep records
  const int C = order <= 0 ? ks : (order >= 3 ? 1 << (order - 3) : 1);
  EXPECT(ks % C == 0);
  std::vector<int> rec_seen(total, 0), src_seen(total, 0);
  int64_t i = 0;
  for (int t = 0; t < T; ++t)
    for (int s = 0; s < ks; ++s)
      for (int h = 0; h < H; ++h)
        for (int l = 0; l < 64; ++l, ++i) {
          const LaneRec r = lane_record<WT_FP4>(i, N, K, rope_rows, D, swiglu, order);
          const int orow = 16 * t + (l & 15) + h * (N / 2);
          int src = orow;
          if (orow < rope_rows) {
            const int hd = orow / D, p = orow % D;
            src = hd * D + p / 2 + (p % 2) * (D / 2);
          }
          const int64_t first = order <= 0 ? ((int64_t)t * ks + s) * (64 * H)
                                           : ((int64_t)(s / C) * T * C + (int64_t)t * C + s % C) * (64 * H);
          EXPECT(r.orow == orow && r.src == src && r.k0 == 128 * s + 32 * (l >> 4));
          EXPECT((int64_t)r.rec == first + h * 64 + l);
          const bool in_range = r.rec < (size_t)total && r.src >= 0 && r.src < N && r.k0 >= 0 && r.k0 + 32 <= K;
          EXPECT(in_range);
          if (!in_range) return;
          ++rec_seen[r.rec];
          ++src_seen[(int64_t)r.src * (K / 32) + r.k0 / 32];
        }
  EXPECT(i == total);
  for (int64_t j = 0; j < total; ++j) EXPECT(rec_seen[j] == 1 && src_seen[j] == 1);
}

static void check_plans() {
  using namespace skinny;
  const SkinnyKnobs kn{};
  const auto plan = [&](int M, int N, int K, int pro, int epi, bool ws, int mode, const SkinnyKnobs& k) {
    return plan_skinny_gemm(WT_FP4, M, N, K, pro, epi, 256, ws, ws ? 256 + 1024 * 528 : 0, mode, k);
  };
  // always one tile per workgroup, whatever the workspace, the split mode, the rows or the knobs
  SkinnyKnobs pinned;
  pinned.splitk = 4, pinned.tn = 4, pinned.alds = 1, pinned.cfg = 808;
  for (const SkinnyKnobs& k : {kn, pinned})
    for (const bool ws : {false, true})
      for (const int M : {1, 3, 16})
        for (const int pro : {PRO_PLAIN, PRO_NORM})
          for (const int epi : {EPI_STORE, EPI_RESID, EPI_SWIGLU, EPI_ROPE}) {
            const int shapes[5][2] = {{6144, 4096}, {4096, 4096}, {14336, 4096}, {4096, 14336}, {768, 4096}};
            for (const auto& sh : shapes) {
              const SkinnyPlan p = plan(M, sh[0], sh[1], pro, epi, ws, 3, k);
              EXPECT(p.rc == 0 && p.form == ONE_TILE && p.grid == sh[0] / 16 && p.NW == 4 && p.block == 256);
              EXPECT(p.U == (sh[0] / 16 >= 384 ? 1 : 2));
              EXPECT(p.TN == 1 && p.MB == 1 && p.S == 1 && p.R == 0 && p.lds_bytes == 0 && !p.alds);
            }
          }
  for (const int epi : {EPI_STORE, EPI_RESID, EPI_SWIGLU, EPI_ROPE})
    EXPECT(plan(3, 4096, 4096, PRO_NORM_ADD, epi, true, 3, kn).rc == -2);
  EXPECT(plan(3, 4096, 4096, PRO_PLAIN, EPI_AR, true, 3, kn).rc == -2);
  EXPECT(!allowed(SPLITK, WT_FP4, PRO_PLAIN, EPI_STORE) && !allowed(MULTI, WT_FP4, PRO_NORM, EPI_STORE) &&
         !allowed(BALANCED, WT_FP4, PRO_NORM, EPI_SWIGLU) && !allowed(ALDS, WT_FP4, PRO_PLAIN, EPI_STORE));
  EXPECT(allowed(ONE_TILE, WT_FP4, PRO_NORM, EPI_RESID));   // which the bf16 one-tile form does not carry
  // the record depth and the chunk rule
  EXPECT(kfrag<WT_FP4>() == 4 && kdeep<WT_FP4>() == 128);
  EXPECT(chunk_log2<WT_FP4>(1) == 0 && chunk_log2<WT_FP4>(2) == 0 && chunk_log2<WT_FP4>(3) == 0 &&
         chunk_log2<WT_FP4>(4) == 1 && chunk_log2<WT_FP4>(5) == 2);
}

static void check_refusals() {
  using namespace skinny;
  EXPECT(weight_shape_ok<WT_FP4>(64, 256, 0, 0, 0) && weight_shape_ok<WT_FP4>(64, 128, 32, 16, 0) &&
         weight_shape_ok<WT_FP4>(64, 128, 0, 0, 1));
  EXPECT(!weight_shape_ok<WT_FP4>(64, 64, 0, 0, 0));     // a multiple of the fp8 record only
  EXPECT(!weight_shape_ok<WT_FP4>(64, 192, 0, 0, 0));
  EXPECT(weight_shape_ok<WT_FP8>(64, 192, 0, 0, 0));
  EXPECT(!weight_shape_ok<WT_FP4>(24, 128, 0, 0, 0) && !weight_shape_ok<WT_FP4>(0, 128, 0, 0, 0) &&
         !weight_shape_ok<WT_FP4>(64, 0, 0, 0, 0));
  EXPECT(!weight_shape_ok<WT_FP4>(48, 128, 0, 0, 1));    // SwiGLU halves of whole tiles
  EXPECT(!weight_shape_ok<WT_FP4>(64, 128, 32, 16, 1) && !weight_shape_ok<WT_FP4>(64, 128, 24, 16, 0) &&
         !weight_shape_ok<WT_FP4>(64, 128, 80, 16, 0) && !weight_shape_ok<WT_FP4>(64, 128, 30, 15, 0));
  // launchers: M outside [1, 16], K not a multiple of 128, N not of 16, missing scale / ROPE operand,
  // a prologue the path does not have: all before any HIP call
  const uint8_t sc[4] = {127, 127, 127, 127};
  const auto gemm = [&](const uint8_t* s, int M, int N, int K, int pro, int epi) {
    return launch_skinny_gemm_fp4(nullptr, nullptr, nullptr, s, nullptr, M, N, K, N, 1e-5f, pro, epi, nullptr, nullptr);
  };
  EXPECT(gemm(sc, 0, 16, 128, 0, 0) == -1);
  EXPECT(gemm(sc, 17, 16, 128, 0, 0) == -1);
  EXPECT(gemm(sc, 3, 16, 64, 0, 0) == -1);
  EXPECT(gemm(sc, 3, 16, 192, 0, 0) == -1);
  EXPECT(gemm(sc, 3, 24, 128, 0, 0) == -1);
  EXPECT(gemm(sc, 3, 0, 128, 0, 0) == -1);
  EXPECT(gemm(nullptr, 3, 16, 128, 0, 0) == -1);
  EXPECT(gemm(sc, 3, 16, 128, 2, 0) == -2);
  EXPECT(gemm(sc, 3, 16, 128, 3, 0) == -2);
  EXPECT(gemm(sc, 3, 16, 128, 1, 3) == -3);
  const auto rope = [&](int M, int K, int Hq, int Hkv, int D, int pro) {
    return launch_skinny_gemm_rope_fp4(nullptr, nullptr, nullptr, sc, M, K, pro, 1e-5f, nullptr, nullptr, nullptr,
                                       nullptr, nullptr, Hq, Hkv, D, 32, nullptr, nullptr);
  };
  EXPECT(rope(17, 128, 2, 1, 32, 1) == -1);
  EXPECT(rope(3, 64, 2, 1, 32, 1) == -1);
  EXPECT(rope(3, 128, 2, 1, 32, 2) == -2);
  EXPECT(rope(3, 128, 2, 1, 48, 1) == -4);   // head_dim off the chunk-major K cache layout
  EXPECT(rope(3, 128, 2, 1, 0, 1) == -1);
  EXPECT(launch_shuffle_weight_fp4(nullptr, nullptr, nullptr, nullptr, 64, 192, 0, 0, 0, nullptr) == -1);
  EXPECT(launch_shuffle_weight_fp4(nullptr, nullptr, nullptr, nullptr, 64, 128, 32, 16, 1, nullptr) == -1);
  EXPECT(launch_shuffle_weight_fp4(nullptr, nullptr, nullptr, nullptr, 24, 128, 0, 0, 0, nullptr) == -1);
  EXPECT(launch_unshuffle_weight_fp4(nullptr, nullptr, nullptr, 64, 64, 0, 0, 0, nullptr) == -1);
  EXPECT(launch_unshuffle_weight_fp4(nullptr, nullptr, nullptr, 64, 128, 24, 16, 0, nullptr) == -1);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: fp4_check <case file>\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "r");
  if (f == nullptr) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  const long n_codes = check_codes(f);
  const long n_scales = check_scales(f);
  long long extra = 0;
  EXPECT(!read_int(f, extra));   // the file holds nothing else
  std::fclose(f);
  int layouts = 0;
  for (int order = 0; order <= 6; ++order) {
    if (!skinny::order_tiles(order, 256)) continue;
    for (const int rope_rows : {0, 32, 64}) check_layout(64, 256, rope_rows, 16, false, order), ++layouts;
    check_layout(64, 256, 0, 16, true, order), ++layouts;
  }
  check_plans();
  check_refusals();
  std::printf("fp4_check: %ld codes, %ld scale bytes, %d layouts, %d failure(s)\n", n_codes, n_scales, layouts,
              failures);
  return failures ? 1 : 0;
}
