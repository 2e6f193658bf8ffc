// Decode-path linear layers (M <= 16 rows, up to 32 with plain / norm prologues): y[M,N] = x[M,K] . W[N,K]^T on MFMA, with the
// layer's elementwise work fused in, so a decode layer needs no separate norm/act kernels.
// The tile code (weight layout, pipeline, prologues, epilogues) lives in skinny_core.h and is
// shared with the persistent decode-layer kernel; the launch decision (form, variant, geometry)
// is the pure plan_skinny_gemm of skinny_plan.h. This file holds the kernel wrappers of every
// form, the (pro, epi) / variant dispatch, the bf16 weight shuffle, and the launchers of both
// weight types (the fp8 quantiser is gemm_skinny_fp8.hip, the mxfp4 one gemm_skinny_fp4.hip).
//
// Fusions (details in skinny_core.h):
//   prologue NORM : RMSNorm with gamma folded into W and 1/rms(x_m) from the same A fragments
//                   (no extra pass, no atomics: deterministic).
//   prologue NORM_ADD: tensor-parallel residual + all-reduced partial, published by workgroup 0.
//   epilogue RESID: res[m,n] = bf16(acc + res[m,n])   (the residual add, in place)
//   epilogue SWIGLU: out[m,n] = silu(acc_gate) * acc_up,  W = [gate(I) ; up(I)]
//   epilogue ROPE  : the qkv projection. Its q/k weight rows are stored pair-interleaved per
//                   head (row 2i <- d=i, row 2i+1 <- d=i+D/2; `shuffle_weight(rope_heads=)`),
//                   so both halves of every rotate-half pair land in the same 16-column tile:
//                   the epilogue rotates them (fp32 cos|sin table), writes q to [M, Hq, D] and
//                   scatters k / v straight into the paged caches (k [blk][h][off][D], v
//                   transposed [blk][h][D][off]). Replaces the K2 rope/cache launch.
#include "skinny_plan.h"

#include <type_traits>
#include <utility>

namespace {
using rt::short8;
using namespace skinny;

// one tile per workgroup; WT_FP8 / WT_FP4: e4m3 / e2m1 weight codes, dequantised in registers (skinny_core.h)
// KV8 (every wrapper below, EPI_ROPE only): the K/V caches are fp8 (skinny_core.h st_kv8)
template <int PRO, int EPI, int NW, int U, int WT = WT_BF16, bool KV8 = false>
__global__ void __launch_bounds__(NW * 64) skinny_gemm_kernel(GemmArgs p) {
  __shared__ GemmSmem<nacc<EPI>(), NW> sm;
  Stage<PRO, EPI, U, WT> st0;
  gemm_tile<PRO, EPI, NW, U, false, false, -1, WT, KV8>(p, blockIdx.x, sm, st0, false, blockIdx.x == 0);
}

// TN tiles per workgroup (skinny_core.h gemm_tiles): serving batches, M > 4
template <int PRO, int EPI, int NW, int U, int TN, int MB = 1, bool KV8 = false>
__global__ void __launch_bounds__(NW * 64) skinny_gemm_multi_kernel(GemmArgs p) {
  // two row blocks x (gate + up) x 4 tiles would not fit the static LDS: that variant is never
  // launched (the plan caps SwiGLU at 2 tiles with two row blocks), compiled as 2 tiles
  constexpr int TNX = (MB == 2 && nacc<EPI>() == 2 && TN > 2) ? 2 : TN;
  __shared__ GemmSmemN<nacc<EPI>(), NW, TNX, MB> sm;
  gemm_tiles<PRO, EPI, NW, U, TNX, MB, KV8>(p, blockIdx.x * TNX, sm);
}


// the dynamic LDS of an ALDS launch: [16] row sums of squares, then the staged rows
RT_DEVICE ALds alds_view(int kspan) {
  extern __shared__ float alds_dyn[];
  return ALds{reinterpret_cast<uint16_t*>(alds_dyn + 16), alds_dyn, kspan + 8};
}

// The same launch with the A operand staged in LDS (skinny_core.h ALDS): tensor-parallel shard
// shapes, where the per-k-step activation loads, not HBM, bound the launch.
template <int PRO, int EPI, int NW, int U, bool KV8 = false>
__global__ void __launch_bounds__(NW * 64) skinny_gemm_alds_kernel(GemmArgs p) {
  __shared__ GemmSmem<nacc<EPI>(), NW> sm;
  Stage<PRO, EPI, U> st0;
  const ALds al = alds_view(p.K);
  gemm_tile<PRO, EPI, NW, U, false, true, -1, WT_BF16, KV8>(p, blockIdx.x, sm, st0, false, blockIdx.x == 0, nullptr,
                                                            &al);
}

// CU-balanced launch for tile counts that are not a multiple of the CU count (gate_up of
// Llama-3-8B / Mistral-7B: 896 tiles on 256 CUs = 3.5 per CU, so half the CUs stream a 4th
// tile while the rest idle): the last R = T mod CUs tiles run as two K-halves each (SplitX in
// skinny_core.h), the other T - R whole. Every CU then gets the same bytes (3 tiles + one
// half-tile at 896/256). Workgroups [0, 2R) are the halves (dispatched first, so their
// hand-offs finish under the whole tiles' streams), [2R, T + R) the whole tiles.
// tools/exp_balance.hip: swiglu 768 / 896 / 1024 tiles = 31.0 / 37.6 / 40.5 us (896 is 1.8 us
// above the line through its neighbours).
template <int PRO, int EPI, int NW, int U, bool KV8 = false>
__global__ void __launch_bounds__(NW * 64) skinny_gemm_bal_kernel(GemmArgs p, int* __restrict__ ws, int R, int xpair) {
  __shared__ GemmSmem<nacc<EPI>(), NW> sm;
  Stage<PRO, EPI, U> st0;
  const int T = p.N / 16;
  const int b = blockIdx.x;
  if (b < 2 * R) {
    // the two halves of a tile on ONE XCD when R % 8 == 0 (blocks b and b + 8 of each group of 16:
    // round-robin dispatch puts both on XCD b % 8), so the combine reads same-XCD partials
    int r, idx;
    if (xpair && (R & 7) == 0) {
      r = (b >> 4) * 8 + (b & 7);
      idx = (b >> 3) & 1;
    } else {
      r = b >> 1;
      idx = b & 1;
    }
    const SplitX sx{reinterpret_cast<float*>(ws + SPLIT_CTRS) + (size_t)r * 2 * SPLIT_STRIDE, ws + r, idx, 2};
    gemm_tile<PRO, EPI, NW, U, false, false, -1, WT_BF16, KV8>(p, T - R + r, sm, st0, false, false, &sx);
  } else {
    gemm_tile<PRO, EPI, NW, U, false, false, -1, WT_BF16, KV8>(p, b - 2 * R, sm, st0, false, false);
  }
}

// Split-K launch for shapes with FEWER tiles than CUs — the tensor-parallel shard GEMMs (Llama-3-8B
// at tp 8: qkv 48 tiles, gate_up 112; tp 4: 96 / 224). One tile per workgroup would stream the
// weights with a fraction of the chip, so every tile's K range is cut into S parts (T x S
// workgroups, SplitX hand-off, last arriver combines in index order and runs the epilogue).
// Placement (speed only, never correctness): with T % 8 == 0 the S parts of a tile get block ids
// b, b + 8, ... — one XCD under round-robin dispatch, so the combine reads same-XCD partials.
// NORM_ADD: every part of tile 0 publishes its K range of x + x2.
template <int PRO, int EPI, int NW, int U, bool ALDS = false, bool KV8 = false>
__global__ void __launch_bounds__(NW * 64) skinny_gemm_splitk_kernel(GemmArgs p, int* __restrict__ ws, int S) {
  __shared__ GemmSmem<nacc<EPI>(), NW> sm;
  Stage<PRO, EPI, U> st0;
  const int T = p.N / 16;
  const int b = blockIdx.x;
  int tile, part;
  if ((T & 7) == 0) {
    const int j = b >> 3;
    tile = (j / S) * 8 + (b & 7);
    part = j % S;
  } else {
    tile = b / S;
    part = b % S;
  }
  const SplitX sx{reinterpret_cast<float*>(ws + SPLIT_CTRS) + (size_t)tile * S * SPLIT_STRIDE, ws + tile, part, S};
  if constexpr (ALDS) {
    const int ks = p.K / 32;
    const ALds al = alds_view(32 * ((ks + S - 1) / S + 1));
    gemm_tile<PRO, EPI, NW, U, false, true, -1, WT_BF16, KV8>(p, tile, sm, st0, false, tile == 0, &sx, &al);
  } else {
    gemm_tile<PRO, EPI, NW, U, false, false, -1, WT_BF16, KV8>(p, tile, sm, st0, false, tile == 0, &sx);
  }
}

// TN tiles per workgroup (gemm_tiles) with each group of TN tiles' K range cut into S parts (SplitX hand-off; group ids dealt as
// in skinny_gemm_splitk_kernel, so a group's parts share an XCD under round-robin dispatch)
template <int PRO, int EPI, int NW, int U, int TN, int MB = 1, bool KV8 = false>
__global__ void __launch_bounds__(NW * 64) skinny_gemm_multi_split_kernel(GemmArgs p, int* __restrict__ ws, int S) {
  __shared__ GemmSmemN<nacc<EPI>(), NW, TN, MB> sm;
  const int G = (p.N / 16 + TN - 1) / TN;
  const int b = blockIdx.x;
  int grp, part;
  if ((G & 7) == 0) {
    const int j = b >> 3;
    grp = (j / S) * 8 + (b & 7);
    part = j % S;
  } else {
    grp = b / S;
    part = b % S;
  }
  const SplitX sx{reinterpret_cast<float*>(ws + SPLIT_CTRS) + (size_t)grp * S * TN * MB * SPLIT_STRIDE, ws + grp, part,
                  S};
  gemm_tiles<PRO, EPI, NW, U, TN, MB, KV8>(p, grp * TN, sm, &sx);
}

int device_cus() {
  static int cache[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (cache[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0;
    cache[dev] = n > 0 ? n : -1;
  }
  return cache[dev] > 0 ? cache[dev] : 0;
}

// Runtime (pro, epi) -> compile-time constants: f(integral_constant PRO, integral_constant EPI)
// runs for the pair if FORM launches it. A pair outside allowed(FORM, WT, ..) is not instantiated
// and returns -2.
template <int FORM, int WT, class F, int... I>
int with_pro_epi(int pro, int epi, F&& f, std::integer_sequence<int, I...>) {
  int rc = -2;
  ([&] {
    constexpr int P = I / 4, E = I % 4;
    if constexpr (allowed(FORM, WT, P, E))
      if (pro == P && epi == E) rc = f(std::integral_constant<int, P>{}, std::integral_constant<int, E>{});
  }(), ...);
  return rc;
}
template <int FORM, int WT, class F>
int with_pro_epi(int pro, int epi, F&& f) {
  return with_pro_epi<FORM, WT>(pro, epi, f, std::make_integer_sequence<int, 12>{});   // 3 prologues x 4 epilogues
}

// The same for the plan's (NW, U, TN, MB): each form lists the variants it is compiled with
template <int NW_, int U_, int TN_ = 1, int MB_ = 1>
struct V {
  static constexpr int NW = NW_, U = U_, TN = TN_, MB = MB_;
};
template <class... Vs, class F>
int with_variant(const SkinnyPlan& pl, F&& f) {
  int rc = -2;
  ((pl.NW == Vs::NW && pl.U == Vs::U && pl.TN == Vs::TN && pl.MB == Vs::MB ? void(rc = f(Vs{})) : void()), ...);
  return rc;
}

template <class... P, class... A>
int launch(void (*kernel)(P...), const SkinnyPlan& pl, hipStream_t stream, A... args) {
  hipLaunchKernelGGL(kernel, dim3(pl.grid), dim3(pl.block), pl.lds_bytes, stream, args...);
  return hipGetLastError() == hipSuccess ? 0 : -6;
}

// KV8: the ROPE epilogue writes an fp8 K/V cache (any other epilogue with it is -2)
template <int WT, bool KV8 = false>
int launch_plan(const SkinnyPlan& pl, const GemmArgs& args, int pro, int epi, int* ws, hipStream_t stream) {
  if constexpr (KV8) {
    if (epi != EPI_ROPE) return -2;
  }
  // the kernels of an fp8 cache exist for the ROPE epilogue only
#define RT_KV8(E) (KV8 && (E) == EPI_ROPE)
  switch (pl.form) {
    case ONE_TILE:
      return with_pro_epi<ONE_TILE, WT>(pro, epi, [&](auto P, auto E) {
        const auto go = [&](auto v) { return launch(skinny_gemm_kernel<P(), E(), v.NW, v.U, WT, RT_KV8(E())>, pl, stream, args); };
        if constexpr (WT == WT_FP8)
          return with_variant<V<4, 2>, V<4, 4>>(pl, go);
        else if constexpr (WT == WT_FP4)
          return with_variant<V<4, 1>, V<4, 2>>(pl, go);
        else
          return with_variant<V<4, 2>, V<16, 2>, V<8, 2>, V<4, 8>, V<8, 4>, V<8, 8>, V<4, 4>>(pl, go);
      });
    case ALDS:
      return with_pro_epi<ALDS, WT>(pro, epi, [&](auto P, auto E) {
        return with_variant<V<4, 2>, V<16, 2>, V<8, 2>, V<4, 8>, V<8, 4>, V<8, 8>, V<4, 4>>(
            pl, [&](auto v) { return launch(skinny_gemm_alds_kernel<P(), E(), v.NW, v.U, RT_KV8(E())>, pl, stream, args); });
      });
    case SPLITK:
      return with_pro_epi<SPLITK, WT>(pro, epi, [&](auto P, auto E) {
        if (pl.alds) return launch(skinny_gemm_splitk_kernel<P(), E(), 8, 2, true, RT_KV8(E())>, pl, stream, args, ws, pl.S);
        return with_variant<V<4, 2>, V<4, 4>, V<8, 2>>(
            pl, [&](auto v) {
              return launch(skinny_gemm_splitk_kernel<P(), E(), v.NW, v.U, false, RT_KV8(E())>, pl, stream, args, ws,
                            pl.S);
            });
      });
    case MULTI:
      return with_pro_epi<MULTI, WT>(pro, epi, [&](auto P, auto E) {
        return with_variant<V<4, 2, 4, 2>, V<4, 2, 2, 2>, V<4, 2, 1, 2>, V<8, 2, 2>, V<4, 4, 2>, V<4, 2, 2>, V<8, 2, 4>,
                            V<4, 2, 4>>(pl, [&](auto v) {
          return launch(skinny_gemm_multi_kernel<P(), E(), v.NW, v.U, v.TN, v.MB, RT_KV8(E())>, pl, stream, args);
        });
      });
    case MULTI_SPLIT:
      return with_pro_epi<MULTI_SPLIT, WT>(pro, epi, [&](auto P, auto E) {
        return with_variant<V<4, 2, 2, 2>, V<4, 2, 2>>(pl, [&](auto v) {
          return launch(skinny_gemm_multi_split_kernel<P(), E(), v.NW, v.U, 2, v.MB, RT_KV8(E())>, pl, stream, args, ws,
                        pl.S);
        });
      });
    case BALANCED:
      return with_pro_epi<BALANCED, WT>(pro, epi, [&](auto P, auto E) {
        return launch(skinny_gemm_bal_kernel<P(), E(), 4, 2, RT_KV8(E())>, pl, stream, args, ws, pl.R, pl.xpair);
      });
  }
#undef RT_KV8
  return -2;
}

// validate -> plan -> fill GemmArgs -> one dispatch on the plan's form. WT_FP8: Ws holds fp8 weight
// codes and wscale their per-row fp32 scales (M <= 16, K % 64 == 0); WT_FP4: Ws holds e2m1 codes and
// wscale their e8m0 block scale bytes in record order (M <= 16, K % 128 == 0); N = output columns
// (SwiGLU: I).
int launch_gemm(int wt, void* out, const void* x, const void* Ws, const void* wscale, void* res, int M, int N, int K,
                int ldo, float eps, int pro, int epi, const void* rope, const void* x2, void* xo, hipStream_t stream,
                int* split_ws, int64_t split_ws_ints, int split_mode, bool kv8 = false) {
  const bool f8 = wt != WT_BF16;   // quantised weights, either type
  const int kd = wt == WT_FP4 ? kdeep<WT_FP4>() : (wt == WT_FP8 ? kdeep<WT_FP8>() : kdeep<WT_BF16>());
  if (!f8 && pro == PRO_NORM_ADD && x2 == nullptr) return -5;
  // 17..32 rows: only the multi-tile launches (two 16-row blocks per MFMA pass)
  if (M < 1 || M > (f8 ? 16 : 32) || K <= 0 || N <= 0 || K % kd || N % 16 || (f8 && wscale == nullptr))
    return -1;
  if (M > 16 && (pro == PRO_NORM_ADD || epi == EPI_AR)) return -1;
  if (f8 && pro != PRO_PLAIN && pro != PRO_NORM) return -2;   // reported ahead of a missing ROPE operand
  RopeEpi re{};
  if (epi == EPI_ROPE) {
    if (rope == nullptr) return -3;
    re = *static_cast<const RopeEpi*>(rope);
    // D % 32: the K write goes through kc_elem ([D/32][BS][32] chunks)
    if (re.D <= 0 || re.D % 32 || N != (re.Hq + 2 * re.Hkv) * re.D) return -4;
    // an fp8 cache: the kc8_elem / vc8_elem block layouts, finite positive scales (-7)
    if (kv8 && (re.D % 64 || re.BS <= 0 || re.BS % 8 || !(re.k_inv > 0.f) || !(re.v_inv > 0.f) ||
                !(re.k_inv <= 3.0e38f) || !(re.v_inv <= 3.0e38f)))
      return -7;
  } else if (kv8) {
    return -7;
  }
  const SkinnyPlan pl =
      plan_skinny_gemm(wt, M, N, K, pro, epi, device_cus(), split_ws != nullptr, split_ws_ints, split_mode, knobs());
  if (pl.rc != 0) return pl.rc;
  GemmArgs args{(uint16_t*)out, (const uint16_t*)x, (const short8*)Ws, (uint16_t*)res, M, N, K, ldo,
                eps, re, (const uint16_t*)x2, (uint16_t*)xo};
  args.kmajor = resolve_order(N / 16, K, epi == EPI_SWIGLU, epi == EPI_ROPE);
  if (wt == WT_FP4) {
    args.bscale = static_cast<const uint8_t*>(wscale);
    return kv8 ? launch_plan<WT_FP4, true>(pl, args, pro, epi, split_ws, stream)
               : launch_plan<WT_FP4>(pl, args, pro, epi, split_ws, stream);
  }
  args.wscale = static_cast<const float*>(wscale);
  if (kv8)
    return f8 ? launch_plan<WT_FP8, true>(pl, args, pro, epi, split_ws, stream)
              : launch_plan<WT_BF16, true>(pl, args, pro, epi, split_ws, stream);
  return f8 ? launch_plan<WT_FP8>(pl, args, pro, epi, split_ws, stream)
            : launch_plan<WT_BF16>(pl, args, pro, epi, split_ws, stream);
}

// Ws[rec] = W[src][k0 .. k0+8) (optionally W * gamma[k] folded in), skinny_core.h lane_record
__global__ void shuffle_kernel(short8* __restrict__ Ws, const uint16_t* __restrict__ W,
                               const uint16_t* __restrict__ gamma, int N, int K, int rope_rows, int D, int swiglu,
                               int order) {
  const int64_t total = lane_records<WT_BF16>(N, K);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const LaneRec r = lane_record<WT_BF16>(i, N, K, rope_rows, D, swiglu != 0, order);
    short8 v = *reinterpret_cast<const short8*>(W + (size_t)r.src * K + r.k0);
    if (gamma != nullptr) {
      const short8 gv = *reinterpret_cast<const short8*>(gamma + r.k0);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (short)rt::f2bf(rt::bf2f((uint16_t)v[j]) * rt::bf2f((uint16_t)gv[j]));
    }
    Ws[r.rec] = v;
  }
}

// Exact inverse of shuffle_kernel's permutation (gamma, if any, stays folded): the row-major
// weight for the prefill GEMMs when only the shuffled copy is kept resident (70B on one GPU).
__global__ void unshuffle_kernel(uint16_t* __restrict__ W, const short8* __restrict__ Ws, int N, int K, int rope_rows,
                                 int D, int swiglu, int order) {
  const int64_t total = lane_records<WT_BF16>(N, K);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const LaneRec r = lane_record<WT_BF16>(i, N, K, rope_rows, D, swiglu != 0, order);
    *reinterpret_cast<short8*>(W + (size_t)r.src * K + r.k0) = Ws[r.rec];
  }
}
}  // namespace

int split_workspace_ints(int max_split_tiles) { return split_words(max_split_tiles); }
int splitk_parts(int T, int ks, int cus, int64_t ws_ints) { return skinny::splitk_parts(T, ks, cus, ws_ints, knobs()); }

int launch_skinny_gemm(void* out, const void* x, const void* Ws, void* res, int M, int N, int K, int ldo, float eps,
                       int pro, int epi, const void* rope, const void* x2, void* xo, hipStream_t stream,
                       int* split_ws, int64_t split_ws_ints, int split_mode) {
  return launch_gemm(WT_BF16, out, x, Ws, nullptr, res, M, N, K, ldo, eps, pro, epi, rope, x2, xo, stream, split_ws,
                     split_ws_ints, split_mode);
}

int launch_skinny_gemm_rope(void* q_out, const void* x, const void* Ws, int M, int K, int pro, float eps,
                            const int64_t* positions, const float* cos_sin, void* k_cache, void* v_cache,
                            const int64_t* slots, int Hq, int Hkv, int D, int BS, const void* x2, void* xo,
                            hipStream_t stream, int* split_ws, int64_t split_ws_ints, int split_mode,
                            const float* bias) {
  const RopeEpi re{positions, cos_sin, (uint16_t*)k_cache, (uint16_t*)v_cache, slots, Hq, Hkv, D, BS, bias};
  return launch_gemm(WT_BF16, q_out, x, Ws, nullptr, nullptr, M, (Hq + 2 * Hkv) * D, K, 0, eps, pro, EPI_ROPE, &re, x2,
                     xo, stream, split_ws, split_ws_ints, split_mode);
}

// fp8 weights (Wq, scale: gemm_skinny_fp8.hip): always one tile per workgroup, no workspace
int launch_skinny_gemm_fp8(void* out, const void* x, const void* Wq, const float* scale, void* res, int M, int N,
                           int K, int ldo, float eps, int pro, int epi, const void* rope, hipStream_t stream) {
  return launch_gemm(WT_FP8, out, x, Wq, scale, res, M, N, K, ldo, eps, pro, epi, rope, nullptr, nullptr, stream,
                     nullptr, 0, 0);
}

int launch_skinny_gemm_rope_fp8(void* q_out, const void* x, const void* Wq, const float* scale, int M, int K, int pro,
                                float eps, const int64_t* positions, const float* cos_sin, void* k_cache,
                                void* v_cache, const int64_t* slots, int Hq, int Hkv, int D, int BS,
                                const float* bias, hipStream_t stream) {
  const RopeEpi re{positions, cos_sin, (uint16_t*)k_cache, (uint16_t*)v_cache, slots, Hq, Hkv, D, BS, bias};
  return launch_skinny_gemm_fp8(q_out, x, Wq, scale, nullptr, M, (Hq + 2 * Hkv) * D, K, 0, eps, pro, EPI_ROPE, &re,
                                stream);
}

// mxfp4 weights (Wq, scale: gemm_skinny_fp4.hip): as the fp8 launches, with one scale BYTE per
// lane record (block of 32 k) instead of one float per row
int launch_skinny_gemm_fp4(void* out, const void* x, const void* Wq, const uint8_t* scale, void* res, int M, int N,
                           int K, int ldo, float eps, int pro, int epi, const void* rope, hipStream_t stream) {
  return launch_gemm(WT_FP4, out, x, Wq, scale, res, M, N, K, ldo, eps, pro, epi, rope, nullptr, nullptr, stream,
                     nullptr, 0, 0);
}

int launch_skinny_gemm_rope_fp4(void* q_out, const void* x, const void* Wq, const uint8_t* scale, int M, int K,
                                int pro, float eps, const int64_t* positions, const float* cos_sin, void* k_cache,
                                void* v_cache, const int64_t* slots, int Hq, int Hkv, int D, int BS,
                                const float* bias, hipStream_t stream) {
  const RopeEpi re{positions, cos_sin, (uint16_t*)k_cache, (uint16_t*)v_cache, slots, Hq, Hkv, D, BS, bias};
  return launch_skinny_gemm_fp4(q_out, x, Wq, scale, nullptr, M, (Hq + 2 * Hkv) * D, K, 0, eps, pro, EPI_ROPE, &re,
                                stream);
}

// The ROPE-epilogue qkv GEMM writing an fp8 K/V cache (kv_dtype "fp8": e4m3fn bytes, value = code *
// scale; common.h kc8_elem / vc8_elem), for all three weight types from the one epilogue: wt = 0
// bf16 (W shuffled, wscale null), 1 fp8 (wscale: fp32 row scales), 2 mxfp4 (wscale: e8m0 bytes).
// x2 / xo / the split workspace: bf16 weights only. -7: scale or cache shape, before any HIP call.
int launch_skinny_gemm_rope_kv8(int wt, void* q_out, const void* x, const void* W, const void* wscale, int M, int K,
                                int pro, float eps, const int64_t* positions, const float* cos_sin, void* k_cache,
                                void* v_cache, const int64_t* slots, int Hq, int Hkv, int D, int BS, const void* x2,
                                void* xo, hipStream_t stream, int* split_ws, int64_t split_ws_ints, int split_mode,
                                const float* bias, float k_scale, float v_scale) {
  if (wt != WT_BF16 && wt != WT_FP8 && wt != WT_FP4) return -1;
  if (!(k_scale > 0.f) || !(v_scale > 0.f) || !(k_scale <= 3.0e38f) || !(v_scale <= 3.0e38f)) return -7;
  RopeEpi re{positions, cos_sin, (uint16_t*)k_cache, (uint16_t*)v_cache, slots, Hq, Hkv, D, BS, bias};
  re.k_inv = 1.f / k_scale;
  re.v_inv = 1.f / v_scale;
  const bool bf = wt == WT_BF16;
  return launch_gemm(wt, q_out, x, W, wscale, nullptr, M, (Hq + 2 * Hkv) * D, K, 0, eps, pro, EPI_ROPE, &re,
                     bf ? x2 : nullptr, bf ? xo : nullptr, stream, bf ? split_ws : nullptr, bf ? split_ws_ints : 0,
                     bf ? split_mode : 0, true);
}

int launch_shuffle_weight(void* Ws, const void* W, const void* gamma, int N, int K, int rope_rows, int D, int swiglu,
                          hipStream_t stream) {
  if (!weight_shape_ok<WT_BF16>(N, K, rope_rows, D, swiglu)) return -1;
  hipLaunchKernelGGL(shuffle_kernel, shuffle_grid(lane_records<WT_BF16>(N, K), 8192), dim3(256), 0, stream,
                     (short8*)Ws, (const uint16_t*)W, (const uint16_t*)gamma, N, K, rope_rows, D, swiglu,
                     shuffle_order(N, K, rope_rows, swiglu));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_unshuffle_weight(void* W, const void* Ws, int N, int K, int rope_rows, int D, int swiglu,
                            hipStream_t stream) {
  if (!weight_shape_ok<WT_BF16>(N, K, rope_rows, D, swiglu)) return -1;
  hipLaunchKernelGGL(unshuffle_kernel, shuffle_grid(lane_records<WT_BF16>(N, K), 65536), dim3(256), 0, stream,
                     (uint16_t*)W, (const short8*)Ws, N, K, rope_rows, D, swiglu,
                     shuffle_order(N, K, rope_rows, swiglu));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
