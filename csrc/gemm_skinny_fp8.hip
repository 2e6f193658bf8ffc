// FP8 weight-only decode GEMMs (W8A16): OCP e4m3fn weight codes with one fp32 scale per weight
// row, bf16 activations, fp32 accumulation on the same v_mfma_f32_16x16x32_bf16 as the bf16 path
// (skinny_core.h, "FP8 weights": record layout, dequantisation in registers, where the scale
// multiplies). Halves the bytes every decode GEMM streams. This file holds
//   - the quantiser + shuffle (two passes: row absmax of W * gamma, then quantise and scatter into
//     fragment order),
//   - the dequantiser + unshuffle (fragment-order codes + scales -> row-major bf16(code * scale),
//     the operand of the prefill / unfused GEMMs),
//   - the one-tile-per-workgroup launches: M <= 16, prologues PLAIN / NORM, epilogues STORE /
//     RESID / SWIGLU / ROPE. No split-K, CU-balanced, multi-tile or all-reduce forms.
//
// Quantiser contract (ops/reference.py quantize_fp8):
//   wf[n,k] = fp32(W[n,k]) * fp32(gamma[k])   (exact in fp32, no bf16 rounding)
//   amax[n] = max_k |wf[n,k]|,  scale[n] = amax[n] / 448  (all-zero row: scale 1, codes 0)
//   code[n,k] = e4m3_rne(clamp(wf[n,k] * (448 / amax[n]), +-448))
// scale[] is stored in the epilogue's column order: ROPE rows pair-interleaved as the codes,
// SwiGLU gate rows [0, I) then up rows [I, 2I).
#include "skinny_core.h"

#include <cstdlib>

namespace {
using rt::short8;
using namespace skinny;

template <int PRO, int EPI, int NW, int U>
__global__ void __launch_bounds__(NW * 64) skinny_gemm_fp8_kernel(GemmArgs p) {
  __shared__ GemmSmem<nacc<EPI>(), NW> sm;
  Stage<PRO, EPI, U, WT_FP8> st0;
  gemm_tile<PRO, EPI, NW, U, false, false, -1, WT_FP8>(p, blockIdx.x, sm, st0, false, false);
}

// RT_WEIGHT_ORDER=0 pins tile-major weights (as gemm_skinny.hip; read once per process). Only 0
// is honoured here: a pinned chunk size is not checked against K.
int forced_order() {
  static const int v = [] {
    const char* e = getenv("RT_WEIGHT_ORDER");
    return e && atoi(e) == 0 ? 0 : -1;
  }();
  return v;
}

// source row of output (epilogue-order) row `row`: the ROPE pair interleave of shuffle_kernel
RT_DEVICE int source_row(int row, int rope_rows, int D) {
  if (row < rope_rows) {
    const int h = row / D, p = row - h * D;
    row = h * D + (p >> 1) + (p & 1) * (D >> 1);
  }
  return row;
}

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

// pass 2: one thread per lane record (16 consecutive k of one row):
// Wq[t][s][l][j] = code(W[16t + (l&15)][64s + 16(l>>4) + j]); SwiGLU k-step-paired as shuffle_kernel
__global__ void fp8_quant_shuffle_kernel(short8* __restrict__ Wq, const float* __restrict__ amax,
                                         const uint16_t* __restrict__ W, const uint16_t* __restrict__ gamma, int N,
                                         int K, int rope_rows, int D, int swiglu, int force_order) {
  const int nsteps = K / 64;
  const int64_t total = (int64_t)(N / 16) * nsteps * 64;
  const int T = swiglu ? N / 32 : N / 16;
  const int order = force_order >= 0 ? force_order : weight_order_fp8(T, K, swiglu != 0, rope_rows > 0);
  const int recs = swiglu ? 128 : 64;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int l = (int)(i & 63);
    int64_t ts = i >> 6;
    int h = 0;
    if (swiglu) {
      h = (int)(ts & 1);
      ts >>= 1;
    }
    const int s = (int)(ts % nsteps);
    const int64_t t = ts / nsteps;
    const int orow = (int)(16 * t + (l & 15)) + h * (N / 2);
    const int row = source_row(orow, rope_rows, D);
    const int k0 = 64 * s + 16 * (l >> 4);
    const float am = amax[orow];
    const float inv = am > 0.f ? 448.f / am : 1.f;
    rt::u32x4 codes;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const short8 v = *reinterpret_cast<const short8*>(W + (size_t)row * K + k0 + 8 * q);
      short8 gv;
      if (gamma != nullptr) gv = *reinterpret_cast<const short8*>(gamma + k0 + 8 * q);
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
    Wq[rec_index_fp8((int)t, s, T, nsteps, order, recs) + h * 64 + l] = __builtin_bit_cast(short8, codes);
  }
}

// inverse: W[src row][k] = bf16(code * scale[row]), rows back in natural order
__global__ void fp8_dequant_unshuffle_kernel(uint16_t* __restrict__ W, const short8* __restrict__ Wq,
                                             const float* __restrict__ scale, int N, int K, int rope_rows, int D,
                                             int swiglu, int force_order) {
  const int nsteps = K / 64;
  const int64_t total = (int64_t)(N / 16) * nsteps * 64;
  const int T = swiglu ? N / 32 : N / 16;
  const int order = force_order >= 0 ? force_order : weight_order_fp8(T, K, swiglu != 0, rope_rows > 0);
  const int recs = swiglu ? 128 : 64;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int l = (int)(i & 63);
    int64_t ts = i >> 6;
    int h = 0;
    if (swiglu) {
      h = (int)(ts & 1);
      ts >>= 1;
    }
    const int s = (int)(ts % nsteps);
    const int64_t t = ts / nsteps;
    const int orow = (int)(16 * t + (l & 15)) + h * (N / 2);
    const int row = source_row(orow, rope_rows, D);
    const int k0 = 64 * s + 16 * (l >> 4);
    const float sc = scale[orow];
    const rt::u32x4 codes =
        __builtin_bit_cast(rt::u32x4, Wq[rec_index_fp8((int)t, s, T, nsteps, order, recs) + h * 64 + l]);
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
      *reinterpret_cast<short8*>(W + (size_t)row * K + k0 + 8 * q) = o;
    }
  }
}

bool fp8_shape_ok(int N, int K, int rope_rows, int D, int swiglu) {
  if (N <= 0 || K <= 0 || K % 64 || N % 16 || rope_rows < 0 || rope_rows > N) return false;
  if (rope_rows > 0 && (D <= 0 || D % 2 || rope_rows % D)) return false;
  if (swiglu && (N % 32 || rope_rows > 0)) return false;
  return true;
}
}  // namespace

// Wq: N*K bytes, scale / amax: N floats each (amax is scratch of the two passes)
int launch_shuffle_weight_fp8(void* Wq, float* scale, float* amax, const void* W, const void* gamma, int N, int K,
                              int rope_rows, int D, int swiglu, hipStream_t stream) {
  if (!fp8_shape_ok(N, K, rope_rows, D, swiglu)) return -1;
  hipLaunchKernelGGL(fp8_amax_kernel, dim3((unsigned)N), dim3(256), 0, stream, amax, scale, (const uint16_t*)W,
                     (const uint16_t*)gamma, K, rope_rows, D);
  const int64_t total = (int64_t)N * K / 16;
  int64_t grid = (total + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(fp8_quant_shuffle_kernel, dim3((unsigned)grid), dim3(256), 0, stream, (short8*)Wq,
                     (const float*)amax, (const uint16_t*)W, (const uint16_t*)gamma, N, K, rope_rows, D, swiglu,
                     forced_order());
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_unshuffle_weight_fp8(void* W, const void* Wq, const float* scale, int N, int K, int rope_rows, int D,
                                int swiglu, hipStream_t stream) {
  if (!fp8_shape_ok(N, K, rope_rows, D, swiglu)) return -1;
  const int64_t total = (int64_t)N * K / 16;
  int64_t grid = (total + 255) / 256;
  if (grid > 65536) grid = 65536;
  hipLaunchKernelGGL(fp8_dequant_unshuffle_kernel, dim3((unsigned)grid), dim3(256), 0, stream, (uint16_t*)W,
                     (const short8*)Wq, scale, N, K, rope_rows, D, swiglu, forced_order());
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// N = output columns (SwiGLU: I, the weight has 2I rows and `scale` 2I entries)
int launch_skinny_gemm_fp8(void* out, const void* x, const void* Wq, const float* scale, void* res, int M, int N,
                           int K, int ldo, float eps, int pro, int epi, const void* rope, hipStream_t stream) {
  if (M < 1 || M > 16 || K <= 0 || K % 64 || N <= 0 || N % 16 || scale == nullptr) return -1;
  if (pro != PRO_PLAIN && pro != PRO_NORM) return -2;
  RopeEpi re{};
  if (epi == EPI_ROPE) {
    if (rope == nullptr) return -3;
    re = *static_cast<const RopeEpi*>(rope);
    if (re.D % 16 || N != (re.Hq + 2 * re.Hkv) * re.D) return -4;
  }
  GemmArgs args{(uint16_t*)out, (const uint16_t*)x, (const short8*)Wq, (uint16_t*)res, M, N, K, ldo,
                eps, re, nullptr, nullptr};
  args.kmajor = forced_order();
  args.wscale = scale;
  const dim3 grid(N / 16);
  // (waves, records per stage) as the bf16 launch of the same shape: the same weight bytes in
  // flight per workgroup
  const bool wide = N / 16 >= 384;
#define RT_F8(P, E)                                                                                      \
  do {                                                                                                   \
    if (wide)                                                                                            \
      hipLaunchKernelGGL((skinny_gemm_fp8_kernel<P, E, 4, 2>), grid, dim3(256), 0, stream, args);        \
    else                                                                                                 \
      hipLaunchKernelGGL((skinny_gemm_fp8_kernel<P, E, 4, 4>), grid, dim3(256), 0, stream, args);        \
  } while (0)
  if (pro == PRO_PLAIN && epi == EPI_STORE) RT_F8(PRO_PLAIN, EPI_STORE);
  else if (pro == PRO_NORM && epi == EPI_STORE) RT_F8(PRO_NORM, EPI_STORE);
  else if (pro == PRO_PLAIN && epi == EPI_RESID) RT_F8(PRO_PLAIN, EPI_RESID);
  else if (pro == PRO_NORM && epi == EPI_RESID) RT_F8(PRO_NORM, EPI_RESID);
  else if (pro == PRO_PLAIN && epi == EPI_SWIGLU) RT_F8(PRO_PLAIN, EPI_SWIGLU);
  else if (pro == PRO_NORM && epi == EPI_SWIGLU) RT_F8(PRO_NORM, EPI_SWIGLU);
  else if (pro == PRO_PLAIN && epi == EPI_ROPE) RT_F8(PRO_PLAIN, EPI_ROPE);
  else if (pro == PRO_NORM && epi == EPI_ROPE) RT_F8(PRO_NORM, EPI_ROPE);
  else return -2;
#undef RT_F8
  return hipGetLastError() == hipSuccess ? 0 : -6;
}

int launch_skinny_gemm_rope_fp8(void* q_out, const void* x, const void* Wq, const float* scale, int M, int K, int pro,
                                float eps, const int64_t* positions, const float* cos_sin, void* k_cache,
                                void* v_cache, const int64_t* slots, int Hq, int Hkv, int D, int BS,
                                const float* bias, hipStream_t stream) {
  const RopeEpi re{positions, cos_sin, (uint16_t*)k_cache, (uint16_t*)v_cache, slots, Hq, Hkv, D, BS, bias};
  return launch_skinny_gemm_fp8(q_out, x, Wq, scale, nullptr, M, (Hq + 2 * Hkv) * D, K, 0, eps, pro, EPI_ROPE, &re,
                                stream);
}
