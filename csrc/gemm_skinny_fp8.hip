// FP8 weight-only decode GEMMs (W8A16): OCP e4m3fn weight codes with one fp32 scale per weight
// row, bf16 activations, fp32 accumulation on the same v_mfma_f32_16x16x32_bf16 as the bf16 path
// (skinny_core.h, "FP8 weights": record layout, dequantisation in registers, where the scale
// multiplies). Halves the bytes every decode GEMM streams. This file holds
//   - the quantiser + shuffle (two passes: row absmax of W * gamma, then quantise and scatter into
//     fragment order),
//   - the dequantiser + unshuffle (fragment-order codes + scales -> row-major bf16(code * scale),
//     the operand of the prefill / unfused GEMMs).
// The GEMM launches are gemm_skinny.hip's (launch_skinny_gemm_fp8: one tile per workgroup,
// M <= 16, prologues PLAIN / NORM, epilogues STORE / RESID / SWIGLU / ROPE; no split-K,
// CU-balanced, multi-tile or all-reduce forms), the record order is the shared lane_record map.
//
// Quantiser contract (ops/reference.py quantize_fp8):
//   wf[n,k] = fp32(W[n,k]) * fp32(gamma[k])   (exact in fp32, no bf16 rounding)
//   amax[n] = max_k |wf[n,k]|,  scale[n] = amax[n] / 448  (all-zero row: scale 1, codes 0)
//   code[n,k] = e4m3_rne(clamp(wf[n,k] * (448 / amax[n]), +-448))
// scale[] is stored in the epilogue's column order: ROPE rows pair-interleaved as the codes,
// SwiGLU gate rows [0, I) then up rows [I, 2I).
#include "skinny_plan.h"

namespace {
using rt::short8;
using namespace skinny;

// pass 1: one workgroup per output row: amax[o] = max_k |W[src(o)][k] * gamma[k]|, scale[o]
__global__ void __launch_bounds__(256) fp8_amax_kernel(float* __restrict__ amax, float* __restrict__ scale,
                                                       const uint16_t* __restrict__ W,
                                                       const uint16_t* __restrict__ gamma, int K, int rope_rows,
                                                       int D) {
  __shared__ float scratch[16];
  const int o = blockIdx.x;
  const uint16_t* wr = W + (size_t)source_row(o, rope_rows, D) * K;
  float m = 0.f;
  for (int k0 = threadIdx.x * 8; k0 < K; k0 += 256 * 8) {
    const short8 v = *reinterpret_cast<const short8*>(wr + k0);
    short8 gv;
    if (gamma != nullptr) gv = *reinterpret_cast<const short8*>(gamma + k0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = rt::bf2f((uint16_t)v[j]);
      if (gamma != nullptr) f *= rt::bf2f((uint16_t)gv[j]);
      m = fmaxf(m, fabsf(f));
    }
  }
  m = rt::block_max(m, scratch);
  if (threadIdx.x == 0) {
    amax[o] = m;
    scale[o] = m > 0.f ? m / 448.f : 1.f;
  }
}

// pass 2: one thread per lane record (16 consecutive k of one row): Wq[rec] = code(W[src][k0 .. k0+16))
__global__ void fp8_quant_shuffle_kernel(short8* __restrict__ Wq, const float* __restrict__ amax,
                                         const uint16_t* __restrict__ W, const uint16_t* __restrict__ gamma, int N,
                                         int K, int rope_rows, int D, int swiglu, int order) {
  const int64_t total = lane_records<WT_FP8>(N, K);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const LaneRec r = lane_record<WT_FP8>(i, N, K, rope_rows, D, swiglu != 0, order);
    const float am = amax[r.orow];
    const float inv = am > 0.f ? 448.f / am : 1.f;
    rt::u32x4 codes;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const short8 v = *reinterpret_cast<const short8*>(W + (size_t)r.src * K + r.k0 + 8 * q);
      short8 gv;
      if (gamma != nullptr) gv = *reinterpret_cast<const short8*>(gamma + r.k0 + 8 * q);
      float y[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = rt::bf2f((uint16_t)v[j]);
        if (gamma != nullptr) f *= rt::bf2f((uint16_t)gv[j]);
        y[j] = fminf(fmaxf(f * inv, -448.f), 448.f);
      }
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        int pk = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * w], y[4 * w + 1], 0, false);
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(y[4 * w + 2], y[4 * w + 3], pk, true);
        codes[2 * q + w] = (unsigned)pk;
      }
    }
    Wq[r.rec] = __builtin_bit_cast(short8, codes);
  }
}

// inverse: W[src row][k] = bf16(code * scale[row]), rows back in natural order
__global__ void fp8_dequant_unshuffle_kernel(uint16_t* __restrict__ W, const short8* __restrict__ Wq,
                                             const float* __restrict__ scale, int N, int K, int rope_rows, int D,
                                             int swiglu, int order) {
  const int64_t total = lane_records<WT_FP8>(N, K);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const LaneRec r = lane_record<WT_FP8>(i, N, K, rope_rows, D, swiglu != 0, order);
    const float sc = scale[r.orow];
    const rt::u32x4 codes = __builtin_bit_cast(rt::u32x4, Wq[r.rec]);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      short8 o;
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        const rt::f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8(codes[2 * q + w], false);
        const rt::f32x2_t b = __builtin_amdgcn_cvt_pk_f32_fp8(codes[2 * q + w], true);
        o[4 * w] = (short)rt::f2bf(a[0] * sc);
        o[4 * w + 1] = (short)rt::f2bf(a[1] * sc);
        o[4 * w + 2] = (short)rt::f2bf(b[0] * sc);
        o[4 * w + 3] = (short)rt::f2bf(b[1] * sc);
      }
      *reinterpret_cast<short8*>(W + (size_t)r.src * K + r.k0 + 8 * q) = o;
    }
  }
}
}  // namespace

// Wq: N*K bytes, scale / amax: N floats each (amax is scratch of the two passes)
int launch_shuffle_weight_fp8(void* Wq, float* scale, float* amax, const void* W, const void* gamma, int N, int K,
                              int rope_rows, int D, int swiglu, hipStream_t stream) {
  if (!weight_shape_ok<WT_FP8>(N, K, rope_rows, D, swiglu)) return -1;
  hipLaunchKernelGGL(fp8_amax_kernel, dim3((unsigned)N), dim3(256), 0, stream, amax, scale, (const uint16_t*)W,
                     (const uint16_t*)gamma, K, rope_rows, D);
  hipLaunchKernelGGL(fp8_quant_shuffle_kernel, shuffle_grid(lane_records<WT_FP8>(N, K), 8192), dim3(256), 0, stream,
                     (short8*)Wq, (const float*)amax, (const uint16_t*)W, (const uint16_t*)gamma, N, K, rope_rows, D,
                     swiglu, shuffle_order(N, K, rope_rows, swiglu));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_unshuffle_weight_fp8(void* W, const void* Wq, const float* scale, int N, int K, int rope_rows, int D,
                                int swiglu, hipStream_t stream) {
  if (!weight_shape_ok<WT_FP8>(N, K, rope_rows, D, swiglu)) return -1;
  hipLaunchKernelGGL(fp8_dequant_unshuffle_kernel, shuffle_grid(lane_records<WT_FP8>(N, K), 65536), dim3(256), 0,
                     stream, (uint16_t*)W, (const short8*)Wq, scale, N, K, rope_rows, D, swiglu,
                     shuffle_order(N, K, rope_rows, swiglu));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
