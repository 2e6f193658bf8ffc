// Host-side argument validation of the HIP launchers, built with AddressSanitizer +
// UndefinedBehaviorSanitizer on the HOST code only (GPU ASan / xnack+ is not
// available on the MI355X pool). Every case below must be rejected BEFORE any HIP call, so
// the binary runs on a machine without a GPU. Build + run: tests/test_native_host_sanitizers.py.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "skinny_plan.h"

int launch_skinny_gemm(void* out, const void* x, const void* Ws, void* res, int M, int N, int K, int ldo, float eps,
                       int pro, int epi, const void* rope, const void* x2, void* xo, hipStream_t stream,
                       int* split_ws, int64_t split_ws_ints, int split_mode);
int splitk_parts(int T, int ks, int cus, int64_t ws_ints);
int launch_shuffle_weight(void* Ws, const void* W, const void* gamma, int N, int K, int rope_rows, int D, int swiglu,
                          hipStream_t stream);
int launch_paged_decode(void* out, const void* q, const void* k_cache, const void* v_cache, const int* block_tables,
                        const int* ctx_lens, float* part_o, float* part_ml, int* counters, int B, int Hq, int Hkv,
                        int D, int max_blocks, float scale, int num_splits, const int* groups, int slot_stride,
                        hipStream_t stream, int defer_combine, int* deferred, const int* plan = nullptr,
                        int plan_stride = 0);
int launch_paging_guard(const int* block_tables, const int* ctx_lens, const int64_t* positions, const int64_t* slots,
                        int* err, int B, int max_blocks, int num_blocks, int BS, hipStream_t stream);
int launch_decode_advance(int64_t* out, int64_t* ids, int64_t* positions, int* ctx_lens, int64_t* step,
                          const int64_t* next, int B, int max_steps, int64_t* slots, int64_t* offsets, void* res,
                          const int* block_tables, const void* embed, int max_blocks, int BS, int H, int64_t vocab,
                          hipStream_t stream);
int prefill32_rows(int G);
int launch_kv_block_copy(void* k, void* v, const int* src, const int* dst, int n, int L, int num_blocks,
                         int64_t block_elems, hipStream_t stream);
int launch_unshuffle_weight(void* W, const void* Ws, int N, int K, int rope_rows, int D, int swiglu,
                            hipStream_t stream);
int launch_skinny_gemm_fp8(void* out, const void* x, const void* Wq, const float* scale, void* res, int M, int N,
                           int K, int ldo, float eps, int pro, int epi, const void* rope, hipStream_t stream);
int launch_shuffle_weight_fp8(void* Wq, float* scale, float* amax, const void* W, const void* gamma, int N, int K,
                              int rope_rows, int D, int swiglu, hipStream_t stream);
int launch_unshuffle_weight_fp8(void* W, const void* Wq, const float* scale, int N, int K, int rope_rows, int D,
                                int swiglu, hipStream_t stream);

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

// The lane-record map (skinny_core.h) on an [N, K] weight: every lane record mapped forward; the
// record offsets must be a permutation of [0, N*K / record) and (source row, k0) must cover the
// matrix exactly once.
template <int WT>
static void check_layout(int N, int K, int rope_rows, int D, bool swiglu, int order) {
  constexpr int kelem = skinny::kdeep<WT>() / 4;   // k elements of one lane record (16 bytes)
  const int64_t total = skinny::lane_records<WT>(N, K);
  EXPECT(total == (int64_t)N * K / kelem);
  std::vector<int> rec_seen(total, 0), src_seen(total, 0);
  for (int64_t i = 0; i < total; ++i) {
    const skinny::LaneRec r = skinny::lane_record<WT>(i, N, K, rope_rows, D, swiglu, order);
    const bool in_range = r.rec < (size_t)total && r.orow >= 0 && r.orow < N && r.src >= 0 && r.src < N &&
                          r.k0 >= 0 && r.k0 % kelem == 0 && r.k0 + kelem <= K;
    EXPECT(in_range);
    if (!in_range) return;
    ++rec_seen[r.rec];
    ++src_seen[(int64_t)r.src * (K / kelem) + r.k0 / kelem];
    // rows outside the ROPE block keep their place; inside it they stay within their head
    EXPECT(r.orow >= rope_rows ? r.src == r.orow : r.src / D == r.orow / D);
  }
  for (int64_t i = 0; i < total; ++i) EXPECT(rec_seen[i] == 1 && src_seen[i] == 1);
}

// plan of a bf16 / fp8 decode GEMM on 256 CUs with the workspace of 1024 split tiles, default knobs
static skinny::SkinnyPlan plan(int wt, int M, int N, int K, int pro, int epi, int split_mode, bool ws = true,
                               const skinny::SkinnyKnobs& kn = skinny::SkinnyKnobs{}) {
  return skinny::plan_skinny_gemm(wt, M, N, K, pro, epi, 256, ws, ws ? 256 + 1024 * 528 : 0, split_mode, kn);
}
static bool is(const skinny::SkinnyPlan& p, int form, int NW, int U, int grid, int TN = 1, int MB = 1, int S = 1,
               int R = 0) {
  return p.rc == 0 && p.form == form && p.NW == NW && p.U == U && p.block == NW * 64 && p.grid == grid &&
         p.TN == TN && p.MB == MB && p.S == S && p.R == R && p.lds_bytes == 0 && !p.alds;
}

static void check_plans() {
  using namespace skinny;
  const int BF = WT_BF16, F8 = WT_FP8;
  // decode (M = 3), Llama-3-8B shapes
  EXPECT(is(plan(BF, 3, 6144, 4096, PRO_NORM, EPI_ROPE, 2), ONE_TILE, 4, 2, 384));
  EXPECT(is(plan(BF, 3, 4096, 4096, PRO_PLAIN, EPI_RESID, 2), ONE_TILE, 4, 4, 256));
  EXPECT(is(plan(BF, 3, 14336, 4096, PRO_NORM, EPI_SWIGLU, 3), BALANCED, 4, 2, 1024, 1, 1, 1, 128));
  EXPECT(is(plan(BF, 3, 14336, 4096, PRO_NORM, EPI_SWIGLU, 2), ONE_TILE, 4, 2, 896));
  EXPECT(is(plan(BF, 3, 4096, 14336, PRO_PLAIN, EPI_RESID, 3), ONE_TILE, 4, 4, 256));
  EXPECT(is(plan(BF, 3, 128256, 4096, PRO_NORM, EPI_STORE, 2), ONE_TILE, 4, 2, 8016));
  // tensor-parallel shards
  EXPECT(is(plan(BF, 3, 3072, 4096, PRO_NORM, EPI_ROPE, 2), ONE_TILE, 8, 2, 192));
  EXPECT(is(plan(BF, 3, 768, 4096, PRO_NORM, EPI_ROPE, 2), SPLITK, 8, 2, 240, 1, 1, 5));
  EXPECT(is(plan(BF, 3, 768, 4096, PRO_NORM, EPI_ROPE, 0), ONE_TILE, 4, 4, 48));
  EXPECT(is(plan(BF, 3, 1792, 4096, PRO_NORM, EPI_SWIGLU, 2), SPLITK, 8, 2, 224, 1, 1, 2));
  // serving batches
  EXPECT(is(plan(BF, 8, 4096, 4096, PRO_PLAIN, EPI_RESID, 2), ONE_TILE, 4, 4, 256));
  EXPECT(is(plan(BF, 16, 6144, 4096, PRO_NORM, EPI_ROPE, 2), MULTI, 4, 2, 192, 2, 1));
  EXPECT(is(plan(BF, 16, 14336, 4096, PRO_NORM, EPI_SWIGLU, 3), MULTI, 4, 2, 224, 4, 1));
  EXPECT(is(plan(BF, 16, 4096, 4096, PRO_PLAIN, EPI_RESID, 2), MULTI_SPLIT, 4, 2, 256, 2, 1, 2));
  EXPECT(is(plan(BF, 16, 4096, 4096, PRO_PLAIN, EPI_RESID, 2, false), ONE_TILE, 4, 4, 256));
  EXPECT(is(plan(BF, 20, 6144, 4096, PRO_NORM, EPI_ROPE, 2), MULTI, 4, 2, 192, 2, 2));
  EXPECT(is(plan(BF, 20, 14336, 4096, PRO_NORM, EPI_SWIGLU, 3), MULTI, 4, 2, 448, 2, 2));
  EXPECT(is(plan(BF, 20, 4096, 4096, PRO_PLAIN, EPI_RESID, 2), MULTI_SPLIT, 4, 2, 256, 2, 2, 2));   // workspace exactly large enough
  // the allowed (pro, epi) sets: bf16 (NORM, RESID) only in the serving-batch forms; NORM_ADD never balanced / multi
  EXPECT(plan(BF, 3, 4096, 4096, PRO_NORM, EPI_RESID, 3).rc == -2);
  EXPECT(plan(BF, 3, 768, 4096, PRO_NORM, EPI_RESID, 3).rc == -2);
  EXPECT(plan(BF, 5, 4096, 4096, PRO_NORM, EPI_RESID, 3).rc == -2);   // 5 rows, but still one tile
  EXPECT(plan(BF, 16, 4096, 4096, PRO_NORM, EPI_RESID, 3).form == MULTI_SPLIT);
  EXPECT(is(plan(BF, 16, 14336, 4096, PRO_NORM_ADD, EPI_SWIGLU, 3), ONE_TILE, 4, 2, 896));
  EXPECT(plan(BF, 3, 4096, 4096, PRO_NORM_ADD, EPI_RESID, 3).rc == -2);
  EXPECT(plan(BF, 3, 4096, 4096, PRO_PLAIN, EPI_AR, 3).rc == -2);
  // fp8: always one tile, no knob, every PLAIN / NORM pair
  EXPECT(is(plan(F8, 3, 6144, 4096, PRO_NORM, EPI_ROPE, 3), ONE_TILE, 4, 2, 384));
  EXPECT(is(plan(F8, 3, 4096, 14336, PRO_NORM, EPI_RESID, 3), ONE_TILE, 4, 4, 256));
  EXPECT(is(plan(F8, 16, 768, 4096, PRO_PLAIN, EPI_SWIGLU, 3), ONE_TILE, 4, 4, 48));
  EXPECT(plan(F8, 3, 4096, 4096, PRO_NORM_ADD, EPI_STORE, 3).rc == -2);
  // every knob still steers the plan
  SkinnyKnobs k;
  k.splitk = 1;
  EXPECT(is(plan(BF, 3, 768, 4096, PRO_NORM, EPI_ROPE, 2, true, k), ONE_TILE, 4, 4, 48));
  k = SkinnyKnobs{}, k.splitk = 3;
  EXPECT(is(plan(BF, 3, 768, 4096, PRO_NORM, EPI_ROPE, 2, true, k), SPLITK, 8, 2, 144, 1, 1, 3));
  k = SkinnyKnobs{}, k.splitk_target = 512;
  EXPECT(is(plan(BF, 3, 768, 4096, PRO_NORM, EPI_ROPE, 2, true, k), SPLITK, 8, 2, 48 * 11, 1, 1, 11));
  k = SkinnyKnobs{}, k.splitk_cfg = 404;
  EXPECT(is(plan(BF, 3, 768, 4096, PRO_NORM, EPI_ROPE, 2, true, k), SPLITK, 4, 4, 240, 1, 1, 5));
  k = SkinnyKnobs{}, k.tn = 1;
  EXPECT(is(plan(BF, 16, 6144, 4096, PRO_NORM, EPI_ROPE, 2, true, k), ONE_TILE, 4, 2, 384));
  k = SkinnyKnobs{}, k.tn = 4;
  EXPECT(is(plan(BF, 16, 6144, 4096, PRO_NORM, EPI_ROPE, 2, true, k), MULTI, 4, 2, 96, 4, 1));
  k = SkinnyKnobs{}, k.tncfg = 802;
  EXPECT(is(plan(BF, 16, 6144, 4096, PRO_NORM, EPI_ROPE, 2, true, k), MULTI, 8, 2, 192, 2, 1));
  k = SkinnyKnobs{}, k.tncfg = 404;   // 4x4 exists for two tiles only
  EXPECT(is(plan(BF, 16, 6144, 4096, PRO_NORM, EPI_ROPE, 2, true, k), MULTI, 4, 4, 192, 2, 1));
  EXPECT(is(plan(BF, 16, 14336, 4096, PRO_NORM, EPI_SWIGLU, 2, true, k), MULTI, 4, 2, 224, 4, 1));
  k = SkinnyKnobs{}, k.tn_minm = 3;
  EXPECT(is(plan(BF, 3, 6144, 4096, PRO_NORM, EPI_ROPE, 2, true, k), MULTI, 4, 2, 192, 2, 1));
  k = SkinnyKnobs{}, k.tns = 0;
  EXPECT(is(plan(BF, 16, 4096, 4096, PRO_PLAIN, EPI_RESID, 2, true, k), ONE_TILE, 4, 4, 256));
  k = SkinnyKnobs{}, k.tns = 2;
  EXPECT(is(plan(BF, 8, 4096, 4096, PRO_PLAIN, EPI_RESID, 2, true, k), MULTI_SPLIT, 4, 2, 256, 2, 1, 2));
  EXPECT(plan(BF, 3, 14336, 4096, PRO_NORM, EPI_SWIGLU, 3).xpair == 1);
  k = SkinnyKnobs{}, k.bal_xcd = 0;
  EXPECT(plan(BF, 3, 14336, 4096, PRO_NORM, EPI_SWIGLU, 3, true, k).xpair == 0);
  k = SkinnyKnobs{}, k.cfg = 804;
  EXPECT(is(plan(BF, 3, 6144, 4096, PRO_NORM, EPI_ROPE, 2, true, k), ONE_TILE, 8, 4, 384));
  k = SkinnyKnobs{}, k.cfg = 303;   // not a compiled variant: 4x4
  EXPECT(is(plan(BF, 3, 6144, 4096, PRO_NORM, EPI_ROPE, 2, true, k), ONE_TILE, 4, 4, 384));
  k = SkinnyKnobs{}, k.alds = 1;   // staged rows: 64 + 3 * (4096 + 8) * 2 bytes of dynamic LDS
  const SkinnyPlan a = plan(BF, 3, 4096, 4096, PRO_PLAIN, EPI_RESID, 2, true, k);
  EXPECT(a.rc == 0 && a.form == ALDS && a.alds && a.NW == 4 && a.U == 4 && a.grid == 256 && a.lds_bytes == 24688);
  const SkinnyPlan as = plan(BF, 3, 768, 4096, PRO_NORM, EPI_ROPE, 2, true, k);   // split-K parts of 26 (+1) k-steps
  EXPECT(as.form == SPLITK && as.alds && as.S == 5 && as.block == 512 && as.lds_bytes == 64 + 3 * (32 * 27 + 8) * 2);
  k = SkinnyKnobs{}, k.alds = 2;   // the shard rule: only with at most one workgroup per CU
  EXPECT(plan(BF, 3, 3072, 4096, PRO_NORM, EPI_ROPE, 2, true, k).form == ALDS);
  EXPECT(plan(BF, 3, 6144, 4096, PRO_NORM, EPI_ROPE, 2, true, k).form == ONE_TILE);
  k.alds = 1;
  EXPECT(plan(BF, 4, 4096, 14336, PRO_PLAIN, EPI_RESID, 0, true, k).form == ONE_TILE);   // 4 rows x 14336 do not fit
  // RT_WEIGHT_ORDER: a pin holds where its chunks tile K, else tile-major; no pin = the shape rule
  EXPECT(resolve_order(256, 14336, false, false, -1) == 1 && resolve_order(384, 4096, false, true, -1) == 3);
  EXPECT(resolve_order(896, 4096, true, false, -1) == 5 && resolve_order(896, 256, true, false, -1) == 0);
  EXPECT(resolve_order(256, 14336, false, false, 0) == 0 && resolve_order(256, 4096, false, false, 3) == 3);
  EXPECT(resolve_order(4, 256, false, false, 4) == 4 && resolve_order(4, 256, false, false, 5) == 0);
  EXPECT(resolve_order(4, 256, false, false, 99) == 0);
}

int main() {
  // decode GEMM: M outside [1, 32] (17..32 only with plain / norm prologues and no all-reduce), K not a
  // multiple of 32, N not a multiple of 16, missing operands
  EXPECT(launch_skinny_gemm(nullptr, nullptr, nullptr, nullptr, 0, 16, 64, 16, 1e-5f, 0, 0, nullptr, nullptr,
                            nullptr, nullptr, nullptr, 0, 3) == -1);
  EXPECT(launch_skinny_gemm(nullptr, nullptr, nullptr, nullptr, 33, 16, 64, 16, 1e-5f, 0, 0, nullptr, nullptr,
                            nullptr, nullptr, nullptr, 0, 3) == -1);
  EXPECT(launch_skinny_gemm(nullptr, nullptr, nullptr, nullptr, 17, 16, 64, 16, 1e-5f, 2, 0, nullptr, nullptr,
                            nullptr, nullptr, nullptr, 0, 3) == -5);   // NORM_ADD without its operand
  EXPECT(launch_skinny_gemm(nullptr, nullptr, nullptr, nullptr, 17, 16, 64, 16, 1e-5f, 2, 0, nullptr, (const void*)1,
                            nullptr, nullptr, nullptr, 0, 3) == -1);   // NORM_ADD above 16 rows
  EXPECT(launch_skinny_gemm(nullptr, nullptr, nullptr, nullptr, 3, 16, 48, 16, 1e-5f, 0, 0, nullptr, nullptr,
                            nullptr, nullptr, nullptr, 0, 3) == -1);
  EXPECT(launch_skinny_gemm(nullptr, nullptr, nullptr, nullptr, 3, 24, 64, 24, 1e-5f, 0, 0, nullptr, nullptr,
                            nullptr, nullptr, nullptr, 0, 3) == -1);
  EXPECT(launch_skinny_gemm(nullptr, nullptr, nullptr, nullptr, 3, 16, 64, 16, 1e-5f, 2, 0, nullptr, nullptr,
                            nullptr, nullptr, nullptr, 0, 3) == -5);   // NORM_ADD without its second operand
  EXPECT(launch_skinny_gemm(nullptr, nullptr, nullptr, nullptr, 3, 16, 64, 16, 1e-5f, 0, 3, nullptr, nullptr,
                            nullptr, nullptr, nullptr, 0, 3) == -3);   // ROPE epilogue without its parameters
  // split-K part choice: only with fewer tiles than CUs, >= 8 k-steps per part, within the workspace
  EXPECT(splitk_parts(384, 128, 256, 1 << 20) == 0);          // tp=1 qkv: tiles >= CUs, no split
  EXPECT(splitk_parts(48, 128, 256, 1 << 20) >= 2);           // tp=8 qkv shard
  EXPECT(splitk_parts(48, 8, 256, 1 << 20) == 0);             // one part of 8 k-steps only
  EXPECT(splitk_parts(48, 128, 256, 256 + 2 * 528 * 48 - 1) == 0);   // workspace below 2 parts
  EXPECT(splitk_parts(100, 128, 0, 1 << 20) == 0);            // unknown CU count
  EXPECT(launch_shuffle_weight(nullptr, nullptr, nullptr, 16, 48, 0, 0, 0, nullptr) == -1);
  EXPECT(launch_shuffle_weight(nullptr, nullptr, nullptr, 32, 64, 64, 128, 0, nullptr) == -1);   // rope rows > N
  EXPECT(launch_shuffle_weight(nullptr, nullptr, nullptr, 48, 64, 0, 0, 1, nullptr) == -1);      // SwiGLU halves of 24 rows
  // decode attention: group size, head dim, split range
  EXPECT(launch_paged_decode(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 30, 8,
                             128, 4, 0.1f, 4, nullptr, 0, nullptr, 0, nullptr) == -1);
  EXPECT(launch_paged_decode(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 64, 2,
                             128, 4, 0.1f, 4, nullptr, 0, nullptr, 0, nullptr) == -1);   // G = 32 > 16
  EXPECT(launch_paged_decode(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 32, 8,
                             128, 4, 0.1f, 65, nullptr, 0, nullptr, 0, nullptr) == -3);  // splits > MAXS
  EXPECT(launch_paged_decode(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 32, 8,
                             128, 4, 0.1f, 4, nullptr, 0, nullptr, 0, nullptr) == 0);    // empty batch: no launch
  static const int grp[3] = {0, 1, 0};
  EXPECT(launch_paged_decode(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2, 32, 8,
                             128, 4, 0.1f, 4, grp, 2, nullptr, 0, nullptr) == -4);   // group slots < splits
  // K8 block copy: empty list launches nothing; unaligned block size / empty layer set refused
  EXPECT(launch_kv_block_copy(nullptr, nullptr, nullptr, nullptr, 0, 32, 16, 8192, nullptr) == 0);
  EXPECT(launch_kv_block_copy(nullptr, nullptr, nullptr, nullptr, 2, 32, 16, 8190, nullptr) == -1);
  EXPECT(launch_kv_block_copy(nullptr, nullptr, nullptr, nullptr, 2, 0, 16, 8192, nullptr) == -1);
  // fp8 launchers: M outside [1, 16], K not a multiple of 64, N not of 16, missing scale / ROPE
  // operand, NORM_ADD; SwiGLU shuffles take no ROPE rows
  const float* sc = (const float*)16;   // never dereferenced on the host
  EXPECT(launch_skinny_gemm_fp8(nullptr, nullptr, nullptr, sc, nullptr, 0, 16, 64, 16, 1e-5f, 0, 0, nullptr, nullptr) == -1);
  EXPECT(launch_skinny_gemm_fp8(nullptr, nullptr, nullptr, sc, nullptr, 17, 16, 64, 16, 1e-5f, 0, 0, nullptr, nullptr) == -1);
  EXPECT(launch_skinny_gemm_fp8(nullptr, nullptr, nullptr, sc, nullptr, 3, 16, 96, 16, 1e-5f, 0, 0, nullptr, nullptr) == -1);
  EXPECT(launch_skinny_gemm_fp8(nullptr, nullptr, nullptr, sc, nullptr, 3, 24, 64, 24, 1e-5f, 0, 0, nullptr, nullptr) == -1);
  EXPECT(launch_skinny_gemm_fp8(nullptr, nullptr, nullptr, nullptr, nullptr, 3, 16, 64, 16, 1e-5f, 0, 0, nullptr, nullptr) == -1);
  EXPECT(launch_skinny_gemm_fp8(nullptr, nullptr, nullptr, sc, nullptr, 3, 16, 64, 16, 1e-5f, 2, 0, nullptr, nullptr) == -2);
  EXPECT(launch_skinny_gemm_fp8(nullptr, nullptr, nullptr, sc, nullptr, 3, 16, 64, 16, 1e-5f, 1, 3, nullptr, nullptr) == -3);
  EXPECT(launch_shuffle_weight_fp8(nullptr, nullptr, nullptr, nullptr, nullptr, 64, 128, 32, 16, 1, nullptr) == -1);
  EXPECT(launch_shuffle_weight_fp8(nullptr, nullptr, nullptr, nullptr, nullptr, 64, 96, 0, 0, 0, nullptr) == -1);
  EXPECT(launch_unshuffle_weight_fp8(nullptr, nullptr, nullptr, 64, 128, 32, 16, 1, nullptr) == -1);
  EXPECT(launch_unshuffle_weight_fp8(nullptr, nullptr, nullptr, 24, 128, 0, 0, 0, nullptr) == -1);
  EXPECT(launch_shuffle_weight(nullptr, nullptr, nullptr, 64, 128, 32, 16, 1, nullptr) == -1);
  EXPECT(launch_unshuffle_weight(nullptr, nullptr, 64, 128, 32, 16, 1, nullptr) == -1);
  // the weight-layout map, N = 64, K = 256: tile-major and every chunked order that tiles K (8
  // bf16 k-steps: chunks of 1, 2, 4, 8), with and without ROPE rows (2 heads of 16), SwiGLU
  for (int order = 0; order <= 4; ++order) {
    EXPECT(skinny::resolve_order(4, 256, false, false, order) == order);
    for (int rope_rows = 0; rope_rows <= 32; rope_rows += 32) {
      check_layout<skinny::WT_BF16>(64, 256, rope_rows, 16, false, order);
      check_layout<skinny::WT_FP8>(64, 256, rope_rows, 16, false, order);
    }
    check_layout<skinny::WT_BF16>(64, 256, 0, 16, true, order);
    check_layout<skinny::WT_FP8>(64, 256, 0, 16, true, order);
  }
  check_plans();
  // weight unshuffle: N%16, K%32, rope rows beyond N
  EXPECT(launch_unshuffle_weight(nullptr, nullptr, 24, 64, 0, 0, 0, nullptr) == -1);
  EXPECT(launch_unshuffle_weight(nullptr, nullptr, 32, 48, 0, 0, 0, nullptr) == -1);
  EXPECT(launch_unshuffle_weight(nullptr, nullptr, 32, 64, 64, 128, 0, nullptr) == -1);
  EXPECT(launch_paging_guard(nullptr, nullptr, nullptr, nullptr, nullptr, 2, 0, 16, 32, nullptr) == -1);
  EXPECT(launch_paging_guard(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 4, 16, 32, nullptr) == 0);
  EXPECT(launch_decode_advance(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 8, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, nullptr) == 0);
  // prefill tile geometry
  // (a group that is not a power of two takes the next power of two of head slots: G = 3 -> 4,
  // G = 7 -> 8; past 8 the 16x16 kernel runs)
  EXPECT(prefill32_rows(4) == 64 && prefill32_rows(8) == 32 && prefill32_rows(1) == 256 && prefill32_rows(3) == 64 &&
         prefill32_rows(7) == 32 && prefill32_rows(5) == 32 && prefill32_rows(12) == 0 && prefill32_rows(16) == 0);
  std::printf("host_check: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
