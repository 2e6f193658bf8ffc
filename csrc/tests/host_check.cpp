// Host-side argument validation of the HIP launchers and the pure host rules behind them (the
// launch plans of skinny_plan.h / attn_plan.h, the weight-layout map, the attention item ranges),
// built with AddressSanitizer + UndefinedBehaviorSanitizer on the HOST code only (SURVEY §5.2;
// GPU ASan / xnack+ is not available on the MI355X pool). Every launcher case below must be
// rejected BEFORE any HIP call, so the binary runs on a machine without a GPU.
// Build + run: tests/test_native_host_sanitizers.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "attn_plan.h"
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

// plan of a decode attention launch, default knobs unless given
static attn::AttnPlan aplan(int B, int Hq, int Hkv, int D, int splits, bool grouped, int stride,
                            const attn::AttnKnobs& kn = attn::AttnKnobs{}, bool defer = false, bool has_plan = false,
                            int plan_stride = 0) {
  return attn::plan_paged_decode(B, Hq, Hkv, D, splits, grouped, stride, has_plan, plan_stride, defer, kn);
}
static bool attn_is(const attn::AttnPlan& p, int gx, int gy, int GM, bool pp, int lm) {
  return p.rc == 0 && p.gx == gx && p.gy == gy && p.splits == gy && p.block == 512 && p.GM == GM && p.pp == pp &&
         p.lm == lm;
}
static bool combine_is(const attn::AttnPlan& p, int nmax, int nsl, int spl, int cgx, int cgy) {
  return p.rc == 0 && p.ext_combine && !p.deferred && p.combine && p.nmax == nmax && p.nsl == nsl && p.spl == spl &&
         p.cblock == 8 * nsl && p.cgx == cgx && p.cgy == cgy;
}
static bool no_combine(const attn::AttnPlan& p, bool ext, bool deferred) {
  return p.rc == 0 && p.ext_combine == ext && p.deferred == deferred && !p.combine;
}

// Expected values worked out by hand from the launcher's rules as they stood before the plan existed.
static void check_attn_plans() {
  using namespace attn;
  // the table (Llama-3-8B tp 1, 3 knights): 4 members x 10 splits = 40 slots -> 2 per lane on 24 lanes
  const AttnPlan t = aplan(3, 32, 8, 128, 10, true, 40);
  EXPECT(attn_is(t, 24, 10, 16, true, 3) && combine_is(t, 40, 24, 2, 96, 4));
  // its tp 8 shard: one kv head keeps the copy loop; 256 slots -> 8 per lane on 32 lanes
  const AttnPlan s8 = aplan(3, 4, 1, 128, 64, true, 256);
  EXPECT(attn_is(s8, 3, 64, 16, false, 3) && combine_is(s8, 256, 32, 8, 12, 4));
  const AttnPlan u = aplan(6, 32, 8, 128, 8, false, 0);
  EXPECT(attn_is(u, 48, 8, 4, true, 3) && combine_is(u, 8, 8, 1, 192, 4));
  EXPECT(no_combine(aplan(6, 32, 8, 128, 1, false, 0), false, false));   // one split: written by the launch
  EXPECT(no_combine(aplan(3, 32, 8, 128, 1, true, 4), false, false));    // grouped, one split: in-launch combine
  // GM: 16 with groups, else by G
  EXPECT(aplan(2, 12, 12, 64, 3, false, 0).GM == 4 && aplan(2, 32, 8, 128, 3, false, 0).GM == 4);
  EXPECT(aplan(2, 20, 4, 128, 3, false, 0).GM == 8 && aplan(2, 28, 4, 128, 3, false, 0).GM == 8);
  EXPECT(aplan(2, 64, 8, 128, 3, false, 0).GM == 8 && aplan(2, 36, 4, 128, 3, false, 0).GM == 16);
  EXPECT(aplan(2, 64, 4, 128, 3, false, 0).GM == 16 && aplan(2, 12, 12, 64, 3, true, 48).GM == 16);
  // D = 64: two 32-dim chunks per combined row
  const AttnPlan d64 = aplan(2, 12, 12, 64, 3, false, 0);
  EXPECT(attn_is(d64, 24, 3, 4, true, 3) && combine_is(d64, 3, 8, 1, 24, 2));
  // return codes, each ahead of every later one: empty batch, head ratio, (splits < 1 clamped,)
  // splits > MAXS, group slots < splits, plan row without ids, head dim
  const AttnPlan e = aplan(0, 30, 8, 100, 65, true, 2, AttnKnobs{}, false, true, 8);
  EXPECT(e.rc == 0 && e.gx == 0 && !e.combine && !e.deferred);
  EXPECT(aplan(2, 30, 8, 100, 65, true, 2, AttnKnobs{}, false, true, 8).rc == -1);
  EXPECT(aplan(2, 64, 2, 100, 65, true, 2, AttnKnobs{}, false, true, 8).rc == -1);   // G = 32 > 16
  EXPECT(attn_is(aplan(2, 32, 8, 128, 0, false, 0), 16, 1, 4, true, 3));
  EXPECT(attn_is(aplan(2, 32, 8, 128, -5, true, 1), 16, 1, 16, true, 3));
  EXPECT(aplan(2, 32, 8, 100, 65, true, 2, AttnKnobs{}, false, true, 8).rc == -3);
  EXPECT(aplan(2, 32, 8, 128, 64, false, 0).rc == 0);
  EXPECT(aplan(2, 32, 8, 100, 4, true, 2, AttnKnobs{}, false, true, 8).rc == -4);
  EXPECT(aplan(2, 32, 8, 100, 4, false, 2, AttnKnobs{}, false, false, 8).rc == -2);   // stride, plan stride unused
  EXPECT(aplan(2, 32, 8, 100, 4, true, 4, AttnKnobs{}, false, true, 8).rc == -5);
  EXPECT(aplan(2, 32, 8, 100, 4, true, 4, AttnKnobs{}, false, true, 9).rc == -2);
  EXPECT(aplan(2, 32, 8, 128, 4, true, 4, AttnKnobs{}, false, true, 9).rc == 0);
  EXPECT(aplan(2, 32, 8, 96, 4, false, 0).rc == -2 && aplan(2, 32, 8, 256, 4, false, 0).rc == -2);
  // defer_combine: the caller combines D = 128 rows; D = 64 keeps the combine launch
  EXPECT(no_combine(aplan(3, 32, 8, 128, 10, true, 40, AttnKnobs{}, true), true, true));
  EXPECT(combine_is(aplan(2, 12, 12, 64, 3, false, 0, AttnKnobs{}, true), 3, 8, 1, 24, 2));
  EXPECT(no_combine(aplan(3, 32, 8, 128, 1, true, 4, AttnKnobs{}, true), false, false));
  // every knob still steers the plan
  AttnKnobs k;
  k.ext_splits = 0;
  EXPECT(no_combine(aplan(3, 32, 8, 128, 10, true, 40, k), false, false));
  EXPECT(no_combine(aplan(3, 32, 8, 128, 10, true, 40, k, true), false, false));
  k = AttnKnobs{}, k.ext_splits = 4;
  EXPECT(no_combine(aplan(6, 32, 8, 128, 3, false, 0, k), false, false));
  EXPECT(combine_is(aplan(6, 32, 8, 128, 4, false, 0, k), 4, 8, 1, 192, 4));
  k = AttnKnobs{}, k.pp = 0;
  EXPECT(attn_is(aplan(3, 32, 8, 128, 10, true, 40, k), 24, 10, 16, false, 3));
  k = AttnKnobs{}, k.pp = 1;
  EXPECT(attn_is(aplan(3, 4, 1, 128, 64, true, 256, k), 3, 64, 16, true, 3));
  EXPECT(aplan(2, 16, 4, 128, 3, false, 0).pp && !aplan(2, 6, 3, 128, 3, false, 0).pp);   // the rule: Hkv >= 4
  for (int lm = 0; lm <= 3; ++lm) {
    k = AttnKnobs{}, k.lm = lm;
    EXPECT(aplan(3, 32, 8, 128, 10, true, 40, k).lm == lm && aplan(3, 4, 1, 128, 64, true, 256, k).lm == lm);
  }
  k = AttnKnobs{}, k.lm = 7;   // the staged loop exists in the ping-pong form only
  EXPECT(aplan(3, 32, 8, 128, 10, true, 40, k).lm == 7 && aplan(3, 4, 1, 128, 64, true, 256, k).lm == 3);
  k.pp = 0;
  EXPECT(aplan(3, 32, 8, 128, 10, true, 40, k).lm == 3);
  k.pp = 1;
  EXPECT(aplan(3, 4, 1, 128, 64, true, 256, k).lm == 7);
  k = AttnKnobs{}, k.lm = 5;
  EXPECT(aplan(3, 32, 8, 128, 10, true, 40, k).lm == 7 && aplan(3, 4, 1, 128, 64, true, 256, k).lm == 1);
  k = AttnKnobs{}, k.skip_combine = true;
  EXPECT(no_combine(aplan(3, 32, 8, 128, 10, true, 40, k), true, false));
  EXPECT(no_combine(aplan(3, 32, 8, 128, 10, true, 40, k, true), true, true));
  k = AttnKnobs{}, k.probe = 2;   // a probe times the in-launch form
  EXPECT(no_combine(aplan(3, 32, 8, 128, 10, true, 40, k), false, false));
  k = AttnKnobs{}, k.combine_nsl = 16;
  EXPECT(combine_is(aplan(3, 32, 8, 128, 10, true, 40, k), 40, 16, 4, 96, 4));
  EXPECT(combine_is(aplan(3, 4, 1, 128, 64, true, 256, k), 256, 16, 8, 12, 4));   // 128 of 256 slots per chunk
  k = AttnKnobs{}, k.combine_nsl = 128;
  EXPECT(combine_is(aplan(3, 32, 8, 128, 10, true, 40, k), 40, 40, 1, 96, 4));
  EXPECT(combine_is(aplan(3, 4, 1, 128, 64, true, 256, k), 256, 128, 2, 12, 4));
  for (const int bad : {0, 4, 20, 136, -8}) {
    k = AttnKnobs{}, k.combine_nsl = bad;
    EXPECT(combine_is(aplan(3, 32, 8, 128, 10, true, 40, k), 40, 24, 2, 96, 4));
  }
  // the slot bound the kernel shares with the plan
  EXPECT(combine_slot_bound(true, 4, 10, 40) == 40 && combine_slot_bound(true, 4, 10, 30) == 30);
  EXPECT(combine_slot_bound(true, 7, 3, 100) == 6 && combine_slot_bound(false, 4, 10, 40) == 10);
  EXPECT(combine_slot_bound(false, 4, 10, 0) == 10 && combine_slot_bound(true, 16, 5, 5) == 5);
}

// the combine launch's geometry against what decode_combine_kernel assumes of it
static void check_combine_geometry() {
  for (const int G : {1, 2, 4, 7, 8, 16})
    for (const int splits : {2, 3, 10, 33, 64})
      for (int grouped = 0; grouped <= 1; ++grouped)
        for (int cap = 8; cap <= 128; cap += 8) {
          attn::AttnKnobs k;
          k.combine_nsl = cap;
          const int stride = grouped ? (16 / G) * splits : 0;
          const attn::AttnPlan p = aplan(2, G, 1, 128, splits, grouped != 0, stride, k);
          const bool ok = p.rc == 0 && p.combine && p.nmax == (grouped ? stride : splits) && p.cblock == 8 * p.nsl &&
                          p.nsl % 8 == 0 && p.nsl >= 8 && p.nsl <= cap && p.cblock <= 1024 &&
                          (p.spl == 1 || p.spl == 2 || p.spl == 4 || p.spl == 8) &&
                          (p.nsl * p.spl >= p.nmax || (p.spl == 8 && p.nsl == cap));   // else: the extra-chunk loop
          EXPECT(ok);
          if (!ok) std::fprintf(stderr, "  G %d splits %d grouped %d cap %d\n", G, splits, grouped, cap);
        }
}

// The items of sequence b (record {first, n, sh}, `ctx` keys) over `splits`: private ranges cover
// [it.sh, ceil(ctx / 32)) exactly once and nothing below; shared chunks are counted into `shared`.
static bool private_cover(int ctx, int first, int n, int sh, bool grouped, int b, int G, int splits,
                          const attn::GroupRec& want, std::vector<int>* shared) {
  const int ntiles = (ctx + 31) / 32;
  std::vector<int> seen(ntiles, 0);
  for (int split = 0; split < splits; ++split) {
    const attn::ItemRange it = attn::item_range(ctx, first, n, sh, grouped, b, split, G, 16, splits);
    if (it.b0 != want.b0 || it.n != want.n || it.sh != want.sh || it.ctx != ctx) return false;
    const int npr = it.nv - it.nsh;   // nv = shared chunk + private tiles
    if (it.nsh < 0 || it.sh_b < 0 || it.sh_b + it.nsh > it.sh || npr < 0 || it.pr_b < it.sh ||
        (npr > 0 && it.pr_b + npr > ntiles))
      return false;
    if (it.nsh > 0 && shared == nullptr) return false;
    for (int t = 0; t < it.nsh; ++t) ++(*shared)[it.sh_b + t];
    for (int t = 0; t < npr; ++t) ++seen[it.pr_b + t];
  }
  for (int t = 0; t < ntiles; ++t)
    if (seen[t] != (t >= want.sh ? 1 : 0)) return false;
  return true;
}

// item_range partitions a group's keys: no gap (keys dropped), no overlap (keys counted twice)
static void check_item_range() {
  const std::vector<std::vector<int>> tail_sets = {{1}, {33}, {0, 1, 500}, {31, 32, 33, 2000}};
  int cases = 0;
  for (const int G : {1, 4, 8, 16})
    for (int n = 1; n <= 16 / G; ++n)
      for (const int splits : {1, 2, 3, 8, 10, 64})
        for (const int sh : {0, 1, 2, 7, 59, 64, 1250})
          for (const auto& tails : tail_sets)
            for (const int first : {0, 2}) {
              std::vector<int> shared(sh, 0);
              bool ok = true;
              for (int i = 0; i < n && ok; ++i) {
                int ctx = sh * 32 + tails[i % tails.size()];
                if (ctx < 1) ctx = 1;
                ok = private_cover(ctx, first, n, sh, true, first + i, G, splits, attn::GroupRec{first, n, sh}, &shared);
              }
              for (int t = 0; t < sh; ++t) ok = ok && shared[t] == 1;   // over all n * splits items
              EXPECT(ok);
              if (!ok) std::fprintf(stderr, "  G %d n %d splits %d sh %d first %d\n", G, n, splits, sh, first);
              ++cases;
            }
  EXPECT(cases == 7728);
  // no record, or a malformed one: the row runs alone over all of its keys
  const int G = 4, b = 3;
  const int bad[][3] = {{2, 0, 5}, {2, -1, 5}, {0, 5, 5}, {-1, 4, 5}, {4, 2, 5}, {0, 3, 5}, {1, 2, 5}, {2, 2, -1}};
  for (const auto& r : bad)
    for (const int ctx : {1, 32, 33, 5000})
      for (const int splits : {1, 3, 64})
        EXPECT(private_cover(ctx, r[0], r[1], r[2], true, b, G, splits, attn::GroupRec{b, 1, 0}, nullptr));
  EXPECT(private_cover(777, 2, 2, 5, false, b, G, 10, attn::GroupRec{b, 1, 0}, nullptr));
  const attn::GroupRec good = attn::group_record(true, 2, 2, 5, b, G);
  EXPECT(good.b0 == 2 && good.n == 2 && good.sh == 5);
  EXPECT(attn::group_record(true, 2, 2, 5, b, G, 4).n == 1);   // LDS for 4 columns only: alone
}

static void check_merge_state() {
  using rt::float4_;
  const auto same = [](float4_ a, float4_ b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3]; };
  const float4_ o2 = {1.f, -2.f, 3.5f, 0.f};
  float M = -INFINITY, L = 0.f;
  float4_ O = {0.f, 0.f, 0.f, 0.f};
  attn::merge_state(M, L, O, 1.5f, 2.f, o2);   // into the empty state: the other state's values
  EXPECT(M == 1.5f && L == 2.f && same(O, o2));
  attn::merge_state(M, L, O, 100.f, 0.f, float4_{9.f, 9.f, 9.f, 9.f});   // a partner without keys is skipped
  attn::merge_state(M, L, O, -INFINITY, 0.f, float4_{0.f, 0.f, 0.f, 0.f});
  EXPECT(M == 1.5f && L == 2.f && same(O, o2));
  attn::merge_state(M, L, O, 2.5f, 1.f, float4_{1.f, 1.f, 1.f, 1.f});    // the larger max rescales the state by 1/2
  EXPECT(M == 2.5f && L == 2.f && same(O, float4_{1.5f, 0.f, 2.75f, 1.f}));
}

int main() {
  check_attn_plans();
  check_combine_geometry();
  check_item_range();
  check_merge_state();
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
