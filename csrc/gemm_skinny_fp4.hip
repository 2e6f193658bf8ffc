// MXFP4 weight-only decode GEMMs (W4A16): OCP e2m1 weight codes with one e8m0 scale byte per block
// of 32 consecutive k of a weight row, bf16 activations, fp32 accumulation on the same
// v_mfma_f32_16x16x32_bf16 as the bf16 path (skinny_core.h, "MXFP4 weights": record layout,
// dequantisation in the convert, where the scale bytes live). 17/32 byte per weight. This file holds
//   - the quantiser + shuffle, ONE pass: a thread owns a lane record, which is a whole scaled
//     block, so the block's amax is thread-local,
//   - the dequantiser + unshuffle (fragment-order codes + record-order scale bytes -> row-major
//     bf16(value(code) * 2^(e-127)), exact; the operand of the prefill / unfused GEMMs).
// The scalar rule (scale byte of an amax, code of a value, value of a code) is fp4_core.h, in plain
// C++ on both sides: the kernels here never use the hardware fp4 converts, so the GEMM's
// v_cvt_scalef32_pk_bf16_fp4 is checked against an independent statement of the format.
// The GEMM launches are gemm_skinny.hip's (launch_skinny_gemm_fp4: one tile per workgroup,
// M <= 16, prologues PLAIN / NORM, epilogues STORE / RESID / SWIGLU / ROPE; no split-K,
// CU-balanced, multi-tile or all-reduce forms), the record order is the shared lane_record map.
//
// Quantiser contract (ops/reference.py quantize_mxfp4):
//   wf[n,k] = fp32(W[n,k]) * fp32(gamma[k])   (exact in fp32, no bf16 rounding)
//   per block of 32 k: e = max(E(amax) - 2, 2); code = sign | nearest e2m1 magnitude of
//   min(|wf| / 2^(e-127), 6), ties to the even code
// Row-major form (the CPU's, and the contract's): byte j of a row = k 2j (low nibble), 2j + 1
// (high). Here the 16 bytes of a lane record are bytes k0/2 .. k0/2 + 15 of its row, and its scale
// is byte `rec` of the scale array.
#include "fp4_core.h"
#include "skinny_plan.h"

namespace {
using rt::short8;
using namespace skinny;

// one thread per lane record: Wq[rec] = codes(W[src][k0 .. k0+32) * gamma), scale[rec] = its byte
__global__ void fp4_quant_shuffle_kernel(short8* __restrict__ Wq, uint8_t* __restrict__ scale,
                                         const uint16_t* __restrict__ W, const uint16_t* __restrict__ gamma, int N,
                                         int K, int rope_rows, int D, int swiglu, int order) {
  const int64_t total = lane_records<WT_FP4>(N, K);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const LaneRec r = lane_record<WT_FP4>(i, N, K, rope_rows, D, swiglu != 0, order);
    float wf[fp4::BLOCK];
    float amax = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const short8 v = *reinterpret_cast<const short8*>(W + (size_t)r.src * K + r.k0 + 8 * q);
      short8 gv;
      if (gamma != nullptr) gv = *reinterpret_cast<const short8*>(gamma + r.k0 + 8 * q);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = rt::bf2f((uint16_t)v[j]);
        if (gamma != nullptr) f *= rt::bf2f((uint16_t)gv[j]);
        wf[8 * q + j] = f;
        amax = fmaxf(amax, fabsf(f));
      }
    }
    const unsigned e = fp4::scale_byte(amax);
    rt::u32x4 codes;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned d = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) d |= fp4::code(wf[8 * q + j], e) << (4 * j);
      codes[q] = d;
    }
    Wq[r.rec] = __builtin_bit_cast(short8, codes);
    scale[r.rec] = (uint8_t)e;
  }
}

// inverse: W[src row][k0 .. k0+32) = bf16(value(code) * 2^(e-127)), rows back in natural order
__global__ void fp4_dequant_unshuffle_kernel(uint16_t* __restrict__ W, const short8* __restrict__ Wq,
                                             const uint8_t* __restrict__ scale, int N, int K, int rope_rows, int D,
                                             int swiglu, int order) {
  const int64_t total = lane_records<WT_FP4>(N, K);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const LaneRec r = lane_record<WT_FP4>(i, N, K, rope_rows, D, swiglu != 0, order);
    const unsigned e = scale[r.rec];
    const rt::u32x4 codes = __builtin_bit_cast(rt::u32x4, Wq[r.rec]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      short8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (short)rt::f2bf(fp4::value((codes[q] >> (4 * j)) & 15u, e));
      *reinterpret_cast<short8*>(W + (size_t)r.src * K + r.k0 + 8 * q) = o;
    }
  }
}
}  // namespace

// Wq: N*K/2 bytes, scale: N*K/32 bytes
int launch_shuffle_weight_fp4(void* Wq, uint8_t* scale, const void* W, const void* gamma, int N, int K,
                              int rope_rows, int D, int swiglu, hipStream_t stream) {
  if (!weight_shape_ok<WT_FP4>(N, K, rope_rows, D, swiglu)) return -1;
  hipLaunchKernelGGL(fp4_quant_shuffle_kernel, shuffle_grid(lane_records<WT_FP4>(N, K), 8192), dim3(256), 0, stream,
                     (short8*)Wq, scale, (const uint16_t*)W, (const uint16_t*)gamma, N, K, rope_rows, D, swiglu,
                     shuffle_order(N, K, rope_rows, swiglu));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_unshuffle_weight_fp4(void* W, const void* Wq, const uint8_t* scale, int N, int K, int rope_rows, int D,
                                int swiglu, hipStream_t stream) {
  if (!weight_shape_ok<WT_FP4>(N, K, rope_rows, D, swiglu)) return -1;
  hipLaunchKernelGGL(fp4_dequant_unshuffle_kernel, shuffle_grid(lane_records<WT_FP4>(N, K), 65536), dim3(256), 0,
                     stream, (uint16_t*)W, (const short8*)Wq, scale, N, K, rope_rows, D, swiglu,
                     shuffle_order(N, K, rope_rows, swiglu));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
