// K2n: per-head QK-norm (Qwen3) + RoPE + paged KV-cache write.
//
// Input is the qkv projection row of each token ([Hq | Hkv | Hkv] x D, bf16, row stride an argument;
// never written). Every q and k head gets an RMSNorm of its own over D, y = x * rsqrt(ss / D + eps) *
// gamma in fp32 (q heads: q_gamma, k heads: k_gamma, both bf16 [D]); y is rotated with the Llama
// rotate-half convention from the host-built fp32 cos|sin row of positions[t], with no rounding to
// bf16 between the norm and the rotation. q leaves as bf16 [T, Hq, D]; k and v go to the paged cache
// exactly as rope_cache.hip writes them (common.h kc_elem / transposed V; KV8: e4m3fn codes of the
// fp32 values times 1/k_scale, 1/v_scale, kv_fp8_core.h, in the kc8_elem / vc8_elem layouts).
//
// One WAVE per (token, head slot), Hq + 2 Hkv slots per token, 4 waves per workgroup (the plan:
// qk_norm_plan.h): a 3-row decode step at 32 / 8 heads is 144 waves on 36 CUs, where one workgroup
// per token would walk 48 heads in turn on 3. Lane l of a q / k wave holds dims l and l + D/2, the
// rotate-half pair, so the rotation needs no lane exchange; D = 64 leaves lanes 32..63 idle. The
// sum of squares is the xor butterfly of common.h wave_sum: a fixed order, the same in every lane.
// A v wave copies (or encodes) its head. No LDS, no barrier: a wave past the end returns at once.
#include "common.h"
#include "kv_fp8_core.h"
#include "qk_norm_plan.h"

namespace {
template <bool ROPE, bool KV8>
__global__ void __launch_bounds__(qkn::THREADS) qk_norm_rope_kernel(
    uint16_t* __restrict__ q_out, const uint16_t* __restrict__ qkv, const int64_t* __restrict__ positions,
    const float* __restrict__ cos_sin, const uint16_t* __restrict__ q_gamma, const uint16_t* __restrict__ k_gamma,
    float eps, uint16_t* __restrict__ k_cache, uint16_t* __restrict__ v_cache, const int64_t* __restrict__ slots,
    int n_waves, int Hq, int Hkv, int D, int BS, int64_t qkv_stride, float k_inv, float v_inv) {
  const int w = blockIdx.x * qkn::WAVES + (threadIdx.x >> 6);
  if (w >= n_waves) return;   // the tail of the last workgroup, before any load
  const int lane = threadIdx.x & 63;
  const int S = Hq + 2 * Hkv;
  const int t = w / S, hs = w - t * S;
  const uint16_t* src = qkv + (size_t)t * qkv_stride + (size_t)hs * D;
  const int half = D >> 1;

  if (hs >= Hq + Hkv) {   // v: transposed store (stride BS)
    const int64_t slot = slots[t];
    const int64_t blk = slot / BS;
    const int off = (int)(slot - blk * BS);
    const int h = hs - Hq - Hkv;
    for (int d = lane; d < D; d += 64) {
      if constexpr (KV8)
        reinterpret_cast<uint8_t*>(v_cache)[((size_t)blk * Hkv + h) * D * BS + rt::vc8_elem(BS, off, d)] =
            (uint8_t)kv_fp8_code(rt::bf2f(src[d]), v_inv);
      else
        v_cache[(((size_t)blk * Hkv + h) * D + d) * BS + off] = src[d];
    }
    return;
  }

  const bool on = lane < half;
  const bool is_k = hs >= Hq;
  const uint16_t* gamma = is_k ? k_gamma : q_gamma;
  float x1 = 0.f, x2 = 0.f, g1 = 0.f, g2 = 0.f;
  if (on) {
    x1 = rt::bf2f(src[lane]);
    x2 = rt::bf2f(src[half + lane]);
    g1 = rt::bf2f(gamma[lane]);
    g2 = rt::bf2f(gamma[half + lane]);
  }
  const float ss = rt::wave_sum(x1 * x1 + x2 * x2);
  const float r = rsqrtf(ss / (float)D + eps);
  float y1 = x1 * r * g1, y2 = x2 * r * g2;
  if constexpr (ROPE) {
    if (on) {
      const float* cs = cos_sin + (size_t)positions[t] * D;
      const float c = cs[lane], s = cs[half + lane];
      const float z1 = y1 * c - y2 * s, z2 = y2 * c + y1 * s;
      y1 = z1;
      y2 = z2;
    }
  }
  if (!on) return;
  if (!is_k) {
    uint16_t* dst = q_out + ((size_t)t * Hq + hs) * D;
    dst[lane] = rt::f2bf(y1);
    dst[half + lane] = rt::f2bf(y2);
    return;
  }
  const int64_t slot = slots[t];
  const int64_t blk = slot / BS;
  const int off = (int)(slot - blk * BS);
  const size_t kblock = ((size_t)blk * Hkv + (hs - Hq)) * BS * D;
  if constexpr (KV8) {
    uint8_t* kb = reinterpret_cast<uint8_t*>(k_cache) + kblock;
    kb[rt::kc8_elem(BS, off, lane)] = (uint8_t)kv_fp8_code(y1, k_inv);
    kb[rt::kc8_elem(BS, off, half + lane)] = (uint8_t)kv_fp8_code(y2, k_inv);
  } else {
    uint16_t* kb = k_cache + kblock;
    kb[rt::kc_elem(BS, off, lane)] = rt::f2bf(y1);
    kb[rt::kc_elem(BS, off, half + lane)] = rt::f2bf(y2);
  }
}

template <bool ROPE, bool KV8>
void launch(int grid, hipStream_t stream, void* q_out, const void* qkv, const int64_t* positions, const float* cos_sin,
            const void* q_gamma, const void* k_gamma, float eps, void* k_cache, void* v_cache, const int64_t* slots,
            int n_waves, int Hq, int Hkv, int D, int BS, int64_t qkv_stride, float k_inv, float v_inv) {
  hipLaunchKernelGGL((qk_norm_rope_kernel<ROPE, KV8>), dim3(grid), dim3(qkn::THREADS), 0, stream, (uint16_t*)q_out,
                     (const uint16_t*)qkv, positions, cos_sin, (const uint16_t*)q_gamma, (const uint16_t*)k_gamma, eps,
                     (uint16_t*)k_cache, (uint16_t*)v_cache, slots, n_waves, Hq, Hkv, D, BS, qkv_stride, k_inv, v_inv);
}
}  // namespace

// ``kv8``: the caches hold one e4m3fn byte per element under k_scale / v_scale (read only then; a
// bf16 launch passes 1). Returns 0, or the plan's negative code before any HIP call.
int launch_qk_norm_rope(void* q_out, const void* qkv, const int64_t* positions, const float* cos_sin,
                        const void* q_gamma, const void* k_gamma, float eps, void* k_cache, void* v_cache,
                        const int64_t* slots, int T, int Hq, int Hkv, int D, int BS, int64_t qkv_stride, bool rope,
                        bool kv8, float k_scale, float v_scale, hipStream_t stream) {
  const bool operands = q_out && qkv && positions && q_gamma && k_gamma && k_cache && v_cache && slots &&
                        (!rope || cos_sin);
  const int grid = qkn::plan(T, Hq, Hkv, D, BS, kv8, k_scale, v_scale, eps, operands);
  if (grid <= 0) return grid;
  const int n_waves = T * (Hq + 2 * Hkv);
  const float ki = 1.f / k_scale, vi = 1.f / v_scale;
#define QKN_LAUNCH(R, K8)                                                                                        \
  launch<R, K8>(grid, stream, q_out, qkv, positions, cos_sin, q_gamma, k_gamma, eps, k_cache, v_cache, slots, n_waves, \
                Hq, Hkv, D, BS, qkv_stride, ki, vi)
  if (rope) {
    if (kv8) QKN_LAUNCH(true, true); else QKN_LAUNCH(true, false);
  } else {
    if (kv8) QKN_LAUNCH(false, true); else QKN_LAUNCH(false, false);
  }
#undef QKN_LAUNCH
  return 0;
}
