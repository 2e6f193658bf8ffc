// K2: fused RoPE + paged KV-cache write.
//
// Input is the fused QKV projection row of each token ([Hq | Hkv | Hkv] x D, bf16).
// q and k are rotated with the Llama rotate-half convention using a host-precomputed
// fp32 cos|sin table (no on-device trig: cdna_hip_programming App. B "Element-wise"),
// q is written to its own [T, Hq, D] tensor, k is scattered to the paged key cache
// (chunk-major blocks, [blk][h][D/32][off][32]: common.h kc_elem) and v to the transposed value cache
// ([blk][h][D][off]) that the MFMA P.V B-operand reads with contiguous loads.
// One workgroup per token; each thread rotates 4 pairs (8-byte loads from both halves).
// KV8 (kv_dtype "fp8"): k and v leave as e4m3fn codes of the fp32 values (the rotation's fp32
// result, never rounded to bf16 first) times 1/k_scale, 1/v_scale (kv_fp8_core.h), in the fp8
// block layouts (common.h kc8_elem / vc8_elem); q stays bf16.
#include "common.h"
#include "kv_fp8_core.h"

namespace {
template <bool ROPE, bool KV8 = false>
__global__ void __launch_bounds__(256) rope_cache_kernel(
    uint16_t* __restrict__ q_out, const uint16_t* __restrict__ qkv, const int64_t* __restrict__ positions,
    const float* __restrict__ cos_sin, uint16_t* __restrict__ k_cache, uint16_t* __restrict__ v_cache,
    const int64_t* __restrict__ slots, int Hq, int Hkv, int D, int BS, int64_t qkv_stride, float k_inv = 1.f,
    float v_inv = 1.f) {
  const int t = blockIdx.x;
  const int64_t slot = slots[t];
  const int64_t blk = slot / BS;
  const int off = (int)(slot - blk * BS);
  const uint16_t* row = qkv + (size_t)t * qkv_stride;
  const int half = D >> 1;
  const int quads = half >> 2;  // 4-pair groups per head
  const float* cs = ROPE ? cos_sin + (size_t)positions[t] * D : nullptr;

  // q and k: (Hq + Hkv) heads x quads
  const int nqk = (Hq + Hkv) * quads;
  for (int i = threadIdx.x; i < nqk; i += blockDim.x) {
    const int h = i / quads;
    const int p = (i - h * quads) * 4;
    const uint16_t* src = row + (size_t)h * D;
    rt::short4 a = *reinterpret_cast<const rt::short4*>(src + p);
    rt::short4 b = *reinterpret_cast<const rt::short4*>(src + half + p);
    rt::short4 oa, ob;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float x1 = rt::bf2f((uint16_t)a[j]), x2 = rt::bf2f((uint16_t)b[j]);
      if constexpr (ROPE) {
        const float c = cs[p + j], s = cs[half + p + j];
        const float y1 = x1 * c - x2 * s, y2 = x2 * c + x1 * s;
        x1 = y1;
        x2 = y2;
      }
      if constexpr (KV8) {
        if (h >= Hq) {   // cache bytes, kept in the low byte of each lane of oa / ob
          oa[j] = (short)kv_fp8_code(x1, k_inv);
          ob[j] = (short)kv_fp8_code(x2, k_inv);
          continue;
        }
      }
      oa[j] = (short)rt::f2bf(x1);
      ob[j] = (short)rt::f2bf(x2);
    }
    if constexpr (KV8) {
      if (h >= Hq) {
        uint8_t* kb = reinterpret_cast<uint8_t*>(k_cache) + ((size_t)blk * Hkv + (h - Hq)) * BS * D;
        const auto pack = [](const rt::short4& c) {
          return (uint32_t)(c[0] & 0xff) | ((uint32_t)(c[1] & 0xff) << 8) | ((uint32_t)(c[2] & 0xff) << 16) |
                 ((uint32_t)(c[3] & 0xff) << 24);
        };
        // 4 dims p..p+3 (p % 4 == 0) never cross a 64-dim chunk
        *reinterpret_cast<uint32_t*>(kb + rt::kc8_elem(BS, off, p)) = pack(oa);
        *reinterpret_cast<uint32_t*>(kb + rt::kc8_elem(BS, off, half + p)) = pack(ob);
        continue;
      }
    }
    // 4 dims p..p+3 (p % 4 == 0) never cross a 32-dim chunk
    uint16_t *da, *db;
    if (h < Hq) {
      da = q_out + ((size_t)t * Hq + h) * D + p;
      db = da + half;
    } else {
      uint16_t* kb = k_cache + ((size_t)blk * Hkv + (h - Hq)) * BS * D;
      da = kb + rt::kc_elem(BS, off, p);
      db = kb + rt::kc_elem(BS, off, half + p);
    }
    *reinterpret_cast<rt::short4*>(da) = oa;
    *reinterpret_cast<rt::short4*>(db) = ob;
  }
  // v: Hkv x D elements, transposed store (stride BS)
  const uint16_t* vsrc = row + (size_t)(Hq + Hkv) * D;
  const int nv = Hkv * D;
  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    const int h = i / D, d = i - h * D;
    if constexpr (KV8)
      reinterpret_cast<uint8_t*>(v_cache)[((size_t)blk * Hkv + h) * D * BS + rt::vc8_elem(BS, off, d)] =
          (uint8_t)kv_fp8_code(rt::bf2f(vsrc[i]), v_inv);
    else
      v_cache[(((size_t)blk * Hkv + h) * D + d) * BS + off] = vsrc[i];
  }
}
}  // namespace

// D must be a multiple of 32 (the K chunks; checked by the binding).
void launch_rope_cache(void* q_out, const void* qkv, const int64_t* positions, const float* cos_sin,
                       void* k_cache, void* v_cache, const int64_t* slots, int T, int Hq, int Hkv, int D, int BS,
                       int64_t qkv_stride, bool rope, hipStream_t stream) {
  if (T == 0) return;
  dim3 grid(T), block(256);
  if (rope)
    hipLaunchKernelGGL((rope_cache_kernel<true>), grid, block, 0, stream, (uint16_t*)q_out, (const uint16_t*)qkv,
                       positions, cos_sin, (uint16_t*)k_cache, (uint16_t*)v_cache, slots, Hq, Hkv, D, BS, qkv_stride);
  else
    hipLaunchKernelGGL((rope_cache_kernel<false>), grid, block, 0, stream, (uint16_t*)q_out, (const uint16_t*)qkv,
                       positions, cos_sin, (uint16_t*)k_cache, (uint16_t*)v_cache, slots, Hq, Hkv, D, BS, qkv_stride);
}

// The same with an fp8 cache (one byte per element): D % 64 == 0 and BS % 8 == 0 (the fp8 block
// layouts), scales finite and > 0. Returns 0, or -1 before any HIP call.
int launch_rope_cache_fp8(void* q_out, const void* qkv, const int64_t* positions, const float* cos_sin,
                          void* k_cache, void* v_cache, const int64_t* slots, int T, int Hq, int Hkv, int D, int BS,
                          int64_t qkv_stride, bool rope, float k_scale, float v_scale, hipStream_t stream) {
  if (T < 0 || Hq < 1 || Hkv < 1 || D <= 0 || D % 64 || BS <= 0 || BS % 8) return -1;
  if (!(k_scale > 0.f) || !(v_scale > 0.f) || !(k_scale <= 3.0e38f) || !(v_scale <= 3.0e38f)) return -1;
  if (rope && cos_sin == nullptr) return -1;
  if (T == 0) return 0;
  if (q_out == nullptr || qkv == nullptr || k_cache == nullptr || v_cache == nullptr || slots == nullptr) return -1;
  dim3 grid(T), block(256);
  const float ki = 1.f / k_scale, vi = 1.f / v_scale;
  if (rope)
    hipLaunchKernelGGL((rope_cache_kernel<true, true>), grid, block, 0, stream, (uint16_t*)q_out,
                       (const uint16_t*)qkv, positions, cos_sin, (uint16_t*)k_cache, (uint16_t*)v_cache, slots, Hq,
                       Hkv, D, BS, qkv_stride, ki, vi);
  else
    hipLaunchKernelGGL((rope_cache_kernel<false, true>), grid, block, 0, stream, (uint16_t*)q_out,
                       (const uint16_t*)qkv, positions, cos_sin, (uint16_t*)k_cache, (uint16_t*)v_cache, slots, Hq,
                       Hkv, D, BS, qkv_stride, ki, vi);
  return 0;
}
