// Host-side launch plan of the decode GEMMs (gemm_skinny.hip): which form runs, with which
// variant and geometry, as a pure function of the shape, the CU count, the workspace and the
// experiment knobs. No HIP calls and no environment reads in plan_skinny_gemm / resolve_order /
// splitk_parts, so csrc/tests/host_check.cpp exercises every rule without a GPU.
#pragma once
#include "skinny_core.h"

#include <cstdio>
#include <cstdlib>

namespace skinny {

constexpr int SPLIT_CTRS = 256;   // counter words at the head of the split workspace
inline int split_words(int split_tiles) { return SPLIT_CTRS + split_tiles * 2 * SPLIT_STRIDE; }

// The experiment knobs (tools/probes, profiles/): read from the environment once per process by
// knobs(), so the shuffles and every launch of one process agree. <NW>x<U> pairs are kept as
// NW * 100 + U.
struct SkinnyKnobs {
  int splitk = 0;          // RT_SPLITK=<S> pins the split-K part count (1 = off)
  int splitk_target = 0;   // RT_SPLITK_TARGET=<wgs>: the r03-first rule S = ceil(wgs / T)
  int splitk_cfg = 802;    // RT_SPLITK_CFG=<NW>x<U> (8x2, 4x2, 4x4): variant of the split-K parts
  int tn = -1;             // RT_SKINNY_TN=<TN> pins the tiles per workgroup (1 = off)
  int tncfg = 402;         // RT_SKINNY_TNCFG=<NW>x<U>: variant of the multi-tile launch
  int tn_minm = 5;         // RT_SKINNY_TN_MINM: the smallest M the multi-tile rule applies to
  int tns = 1;             // RT_SKINNY_TNS: 0 keeps one tile, 2 forces the two-tile K-split below 9 rows
  int bal_xcd = 1;         // RT_BAL_XCD=0: halves of a remainder tile on adjacent block ids (r02)
  int cfg = 0;             // RT_SKINNY_CFG=<NW>x<U> (4x2, 8x2, 4x4, 8x4, 8x8, 4x8, 16x2) pins the one-tile variant
  int alds = 0;            // RT_GEMM_ALDS: 1 whenever the staged rows fit, 2 = the "shard shapes" rule
  int weight_order = -1;   // RT_WEIGHT_ORDER=<order> pins the weight record order (0 = tile-major)
};
inline const SkinnyKnobs& knobs() {
  static const SkinnyKnobs k = [] {
    SkinnyKnobs k;
    const auto num = [](const char* name, int dflt) {
      const char* e = getenv(name);
      return e ? atoi(e) : dflt;
    };
    const auto pair = [](const char* name, int dflt) {
      const char* e = getenv(name);
      int nw = 0, u = 0;
      return e && sscanf(e, "%dx%d", &nw, &u) == 2 ? nw * 100 + u : dflt;
    };
    k.splitk = num("RT_SPLITK", k.splitk);
    k.splitk_target = num("RT_SPLITK_TARGET", k.splitk_target);
    k.splitk_cfg = pair("RT_SPLITK_CFG", k.splitk_cfg);
    k.tn = num("RT_SKINNY_TN", k.tn);
    k.tncfg = pair("RT_SKINNY_TNCFG", k.tncfg);
    k.tn_minm = num("RT_SKINNY_TN_MINM", k.tn_minm);
    k.tns = num("RT_SKINNY_TNS", k.tns);
    const char* x = getenv("RT_BAL_XCD");
    k.bal_xcd = !(x && x[0] == '0');
    k.cfg = pair("RT_SKINNY_CFG", k.cfg);
    k.alds = num("RT_GEMM_ALDS", k.alds);
    k.weight_order = num("RT_WEIGHT_ORDER", k.weight_order);
    return k;
  }();
  return k;
}

// The record order of a T-tile x K weight (T counts output tiles: I / 16 for SwiGLU): the pin
// (RT_WEIGHT_ORDER, A/B against the shape rule) if it is set, else the shape's rule. A pinned
// chunk that does not tile K falls back to tile-major, as the rule itself does. The shuffles and
// every GEMM launch take the order from here, so they cannot disagree.
inline int resolve_order(int T, int K, bool swiglu, bool rope, int pin) {
  if (pin < 0) return weight_order(T, K, swiglu, rope);
  return order_tiles(pin, K) ? pin : 0;
}
inline int resolve_order(int T, int K, bool swiglu, bool rope) {
  return resolve_order(T, K, swiglu, rope, knobs().weight_order);
}
// ... of the [N, K] weight a shuffle / unshuffle is given (SwiGLU: N = 2I rows)
inline int shuffle_order(int N, int K, int rope_rows, int swiglu) {
  return resolve_order((swiglu ? N / 2 : N) / 16, K, swiglu != 0, rope_rows > 0);
}

// One layout check for shuffle and unshuffle of both weight types: N rows (SwiGLU: [gate; up]
// halves of whole tiles), K a whole number of records, ROPE rows whole heads of even size.
template <int WT>
inline bool weight_shape_ok(int N, int K, int rope_rows, int D, int swiglu) {
  if (N <= 0 || K <= 0 || K % kdeep<WT>() || N % 16 || rope_rows < 0 || rope_rows > N) return false;
  if (rope_rows > 0 && (D <= 0 || D % 2 || rope_rows % D)) return false;
  if (swiglu && (N % 32 || rope_rows > 0)) return false;
  return true;
}

// grid of a shuffle / unshuffle launch: 256 lane records per workgroup, grid-stride above `cap`
inline dim3 shuffle_grid(int64_t records, int64_t cap) {
  const int64_t g = (records + 255) / 256;
  return dim3((unsigned)(g < cap ? g : cap));
}

enum Form : int { ONE_TILE, ALDS, SPLITK, MULTI, MULTI_SPLIT, BALANCED };

// The (pro, epi) pairs each form launches. bf16 one-tile, ALDS and split-K carry the three
// NORM_ADD pairs and no (NORM, RESID); the serving-batch forms take PLAIN / NORM with every
// epilogue; the CU-balanced form is not for NORM_ADD (its workgroup 0 publishes the whole K
// row). fp8 and mxfp4 weights: one tile, PLAIN / NORM, every epilogue.
constexpr bool allowed(int form, int wt, int pro, int epi) {
  if (pro < PRO_PLAIN || pro > PRO_NORM_ADD || epi < EPI_STORE || epi > EPI_ROPE) return false;
  if (wt != WT_BF16) return form == ONE_TILE && pro != PRO_NORM_ADD;
  if (form == MULTI || form == MULTI_SPLIT) return pro != PRO_NORM_ADD;
  if (epi == EPI_RESID) return pro == PRO_PLAIN;
  return form != BALANCED || pro != PRO_NORM_ADD;
}

struct SkinnyPlan {
  int rc = 0;          // 0, or -2: the form has no kernel for (pro, epi)
  int form = ONE_TILE;
  int NW = 4, U = 4;   // waves per workgroup, k-steps per pipeline stage
  int TN = 1, MB = 1;  // tiles per workgroup, 16-row blocks (MULTI, MULTI_SPLIT)
  int S = 1;           // K parts per tile or tile group (SPLITK, MULTI_SPLIT)
  int R = 0;           // remainder tiles run as two K halves (BALANCED)
  int grid = 0, block = 256;
  int lds_bytes = 0;   // dynamic LDS (the staged A rows)
  bool alds = false;   // A operand staged in LDS (ALDS, or SPLITK with the knob)
  int xpair = 0;       // BALANCED: the two halves of a tile on one XCD
};

// ALDS decision (skinny_core.h): RT_GEMM_ALDS=1 whenever the staged rows fit, =2 when they fit
// and the launch has at most one workgroup per CU, unset / 0 never. Staged rows + row sums
// <= 48 KB, so the workgroup stays under 64 KB of LDS.
// default OFF: measured slower than the pipelined activation loads on every shard shape except
// the NORM_ADD prologue, which the decode path no longer uses (tools/probes/gemm_variants.py,
// profiles/r04/gemm_variants.md); RT_GEMM_ALDS=1 forces it, =2 is the "shard shapes" rule
constexpr int ALDS_MAX_BYTES = 48 * 1024;
inline bool use_alds(int M, int kspan, int wgs, int cus, int mode) {
  if (mode == 0 || alds_bytes(M, kspan) > ALDS_MAX_BYTES) return false;
  return mode == 1 || (mode == 2 && cus > 0 && wgs <= cus);
}

// Split-K part count for a T-tile, ks-k-step GEMM on `cus` CUs (0 = no split-K): the most parts
// that keep every CU at one workgroup (profiles/r03/gemm_tp_shards_*), each part >= 8 k-steps,
// T x S capped by the workspace. RT_SPLITK=<S> pins S (1 = off),
// RT_SPLITK_TARGET=<wgs> = the r03-first rule S = ceil(wgs / T) (microbenchmark sweeps).
inline int splitk_parts(int T, int ks, int cus, int64_t ws_ints, const SkinnyKnobs& kn) {
  if (cus <= 0 || T >= cus || T > SPLIT_CTRS || kn.splitk == 1) return 0;
  const int smax = ks / 8 < 16 ? ks / 8 : 16;
  int S;
  if (kn.splitk > 1) {
    S = kn.splitk;
  } else if (kn.splitk_target > 0) {
    S = (kn.splitk_target + T - 1) / T;
  } else {
    // at most ONE part per CU: T x S just above the CU count doubles some CUs, which costs more
    // than the split gains (r03 microbench, Llama-3-8B shards, us unsplit -> split: tp 8 qkv 48
    // tiles 8.70 -> 8.34 at S = 6 (288 WGs) / 11.26 at S = 11; tp 2 qkv 192 tiles 9.44 -> 10.85 at
    // S = 2; tp 4 gate_up 224 tiles 13.64 -> 14.18 at S = 2): S = floor(cus / T), so only shapes
    // with <= cus / 2 tiles split
    S = cus / T;
  }
  S = S < smax ? S : smax;
  while (S >= 2 && SPLIT_CTRS + (int64_t)T * S * SPLIT_STRIDE > ws_ints) --S;
  return S >= 2 ? S : 0;
}

// The launch of one validated decode GEMM: N = output columns (SwiGLU: I), M <= 32 (fp8, mxfp4: 16).
// `have_split_ws` / `split_ws_ints`: the caller's split workspace; split_mode bit 0 allows the
// CU-balanced form, bit 1 split-K.
inline SkinnyPlan plan_skinny_gemm(int wt, int M, int N, int K, int pro, int epi, int cus, bool have_split_ws,
                                   int64_t split_ws_ints, int split_mode, const SkinnyKnobs& kn) {
  SkinnyPlan pl;
  const int T = N / 16;
  const auto done = [&](int form, int cfg, int grid) {
    pl.form = form;
    pl.NW = cfg / 100;
    pl.U = cfg % 100;
    pl.grid = grid;
    pl.block = pl.NW * 64;
    pl.rc = allowed(form, wt, pro, epi) ? 0 : -2;
    return pl;
  };
  // fp8 weights: one tile per workgroup; (waves, records per stage) as the bf16 launch of the
  // same shape: the same weight bytes in flight per workgroup
  if (wt == WT_FP8) return done(ONE_TILE, T >= 384 ? 402 : 404, T);
  // mxfp4 weights: one tile per workgroup. A 128-deep record brings four activation fragments, so
  // the fp8 launch's k range per stage is half its record count: 4 waves x 1 record for the wide
  // GEMMs, x 2 for the rest (the same activation bytes in flight as fp8, half the weight bytes).
  // The first form only: not tuned
  if (wt == WT_FP4) return done(ONE_TILE, T >= 384 ? 401 : 402, T);
  // split-K (split_mode bit 1) when the shape has fewer tiles than CUs: tensor-parallel shards
  if (have_split_ws && (split_mode & 2) && M <= 16) {
    const int S = splitk_parts(T, K / 32, cus, split_ws_ints, kn);
    if (S >= 2) {
      // (NW, U) of the split-K parts: 8 waves x 2 steps — one part per CU streams with twice
      // the bytes in flight of 4 waves (r03 microbench, Llama-3-8B tp 4 qkv 8.79 -> 7.98 us; tp 2/8
      // shards within noise; 4x4 no better: profiles/r03/gemm_tp_splitk_cfg_sweep.md).
      // RT_SPLITK_CFG=<NW>x<U> (8x2, 4x2, 4x4) pins it
      const int cfg = kn.splitk_cfg == 402 || kn.splitk_cfg == 404 ? kn.splitk_cfg : 802;
      const int kspan = 32 * ((K / 32 + S - 1) / S + 1);
      pl.S = S;
      pl.alds = cfg == 802 && use_alds(M, kspan, T * S, cus, kn.alds);
      pl.lds_bytes = pl.alds ? alds_bytes(M, kspan) : 0;
      return done(SPLITK, cfg, T * S);
    }
  }
  // Serving batches (M > 4): TN tiles per workgroup share each activation fragment (skinny_core.h
  // gemm_tiles), as long as the launch still covers 3/4 of the CUs. MI355X, Llama-3-8B, M = 16
  // (profiles/r05/gemm_multi_tile.md): lm_head 235.0 -> 163.2 us (TN 4), gate_up 42.1 -> 38.7
  // (TN 4), qkv 16.7 -> 13.5 (TN 2); o / down (256 tiles) lose with fewer workgroups and keep one
  // tile. RT_SKINNY_TN=<TN> (1 = off) pins the tile count, RT_SKINNY_TNCFG=<NW>x<U> the variant
  // (microbenchmarks); the M <= 4 decode path is unchanged.
  // A/B knob: the smallest M the multi-tile rule applies to (M = 3 gains nothing: the activation
  // fragments of 3 rows are L1 hits, profiles/r05/gemm_multi_tile.md); RT_SKINNY_TNS=2 forces the
  // two-tile K-split below 9 rows.
  // 17..32 rows: only these launches (two 16-row blocks per MFMA pass)
  if ((M >= kn.tn_minm || M > 16) && (pro == PRO_PLAIN || pro == PRO_NORM) && epi != EPI_AR) {
    pl.MB = M > 16 ? 2 : 1;
    const int need = cus * 3 / 4;
    int tn = kn.tn >= 0 ? kn.tn : (cus <= 0 ? 1 : (T / 4 >= need ? 4 : (T / 2 >= need ? 2 : 1)));
    // LDS: two row blocks x (gate + up) x 4 tiles would not fit
    if (pl.MB == 2) tn = tn >= 4 && epi != EPI_SWIGLU ? 4 : (tn >= 2 ? 2 : 1);
    // one tile per workgroup would still fill the chip (o / down: 256 tiles): two tiles per
    // workgroup over two K halves keep the workgroup count and halve the activation reads — from
    // 9 rows on (M = 16: down 28.8 -> 23.6 us, o 11.0 -> 10.6; M = 8: o 8.8 -> 10.0, down even,
    // profiles/r05/gemm_multi_tile.md). RT_SKINNY_TNS=0 keeps one tile.
    const int G2 = (T + 1) / 2;
    if (tn == 1 && kn.tn < 0 && kn.tns && (M > 8 || kn.tns == 2) && cus > 0 && T >= need && G2 <= SPLIT_CTRS &&
        K / 32 >= 32 && have_split_ws &&
        split_ws_ints >= (int64_t)SPLIT_CTRS + (int64_t)G2 * 2 * 2 * pl.MB * SPLIT_STRIDE) {
      pl.TN = 2;
      pl.S = 2;
      return done(MULTI_SPLIT, 402, G2 * 2);
    }
    if (tn == 2 || tn == 4 || pl.MB == 2) {
      pl.TN = tn;
      int cfg = 402;
      if (pl.MB == 1 && (kn.tncfg == 802 || (kn.tncfg == 404 && tn == 2))) cfg = kn.tncfg;
      return done(MULTI, cfg, (T + tn - 1) / tn);
    }
    pl.MB = 1;
  }
  // CU-balanced variant (split_mode bit 0): whole plain/norm tiles + split remainder (not for
  // NORM_ADD, whose workgroup 0 publishes the whole K row). ROPE finishes its pairs after the
  // hand-off (partner = adjacent lane's combined sum); the decode path does not use it for qkv:
  // Llama-3-8B qkv (384 tiles) measured 11.02 us plain vs 12.28 us balanced
  // (profiles/experiments/README_r02.md)
  if (have_split_ws && (split_mode & 1) && pro != PRO_NORM_ADD && (K / 32) % 2 == 0 && K >= 64) {
    const int R = cus > 0 ? T % cus : 0;
    if (cus > 0 && T > cus && R > 0 && R <= SPLIT_CTRS && split_ws_ints >= split_words(R)) {
      pl.R = R;
      // the two halves of a remainder tile on one XCD (RT_BAL_XCD=0: adjacent block ids, r02)
      pl.xpair = kn.bal_xcd;
      return done(BALANCED, 402, T + R);
    }
  }
  // Variant = (waves per workgroup NW, k-steps per stage U). Since the pipeline's waits are
  // counted (skinny_core.h gemm_tile), 4 waves win on every decode shape: U = 2 for the wide
  // GEMMs (>= 384 column tiles: qkv 11.5, gate_up 39.0 us), U = 4 for the 256-tile o / down
  // (8.05 / 20.9 us; U = 2 loses there) — profiles/r01_microbench_v3_cfg_sweep.log, v4, v5
  // (4x1, 2x2, 2x4 lose on every shape).
  // Before the counted waits the narrow projections needed 8 waves to keep bytes in flight.
  // RT_SKINNY_CFG=<NW>x<U> (4x2, 8x2, 4x4, 8x4, 8x8, 4x8, 16x2) pins one for microbenchmarks;
  // any other value runs 4x4.
  // 129-224 tiles of >= 64 KB (tensor-parallel shards: tp2 qkv 192 tiles) stream on most of the
  // CUs: 8 waves keep twice the bytes in flight per CU (tp2 qkv norm+rope 7.86 -> 7.34 us;
  // tools/probes/stream_probe.hip 192 x 128 KB 8x2 6.53 / 4x4 6.99 us). Fewer tiles (48-96) stay
  // at 4 x 4: 16 x 2 streams faster there in the probe (48 x 128 KB 5.32 vs 6.00 us) but loses in
  // the GEMM (tp8 qkv 6.74 -> 7.24 us: the 16-wave LDS reduction and epilogue).
  int cfg = T >= 384 ? 402 : 404;
  if (K >= 2048 && T > 128 && T <= 224) cfg = 802;
  if (kn.cfg) {
    cfg = 404;
    for (const int c : {402, 1602, 802, 408, 804, 808})
      if (kn.cfg == c) cfg = c;
  }
  pl.alds = !kn.cfg && use_alds(M, K, T, cus, kn.alds);
  pl.lds_bytes = pl.alds ? alds_bytes(M, K) : 0;
  return done(pl.alds ? ALDS : ONE_TILE, cfg, T);
}

}  // namespace skinny
