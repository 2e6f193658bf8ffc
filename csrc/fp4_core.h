// The scalar rule of the MXFP4 weight format (OCP e2m1 codes + one e8m0 scale byte per block of 32
// consecutive k of one weight row; ops/reference.py quantize_mxfp4 / dequantize_mxfp4 is the
// contract). __host__ __device__: the quantise / dequantise kernels of gemm_skinny_fp4.hip and the
// host check (csrc/tests/fp4_check.cpp) run the same copy.
//
//   scale byte   e = max(E - 2, 2), E the fp32 exponent field of the block's largest |wf|: the OCP
//                rule floor(log2 amax) - emax(e2m1), floored so that 0.5 * 2^(e-127) is a normal
//                bf16; E <= 254 keeps 6 * 2^(e-127) finite. An all-zero block: e = 2, codes 0.
//   code         y = |wf| / 2^(e-127) (exact), low three bits = the e2m1 magnitude
//                {0, 0.5, 1, 1.5, 2, 3, 4, 6} nearest to min(y, 6), ties to the even code; bit 3 =
//                the sign bit of wf, always (a negative value that rounds to zero is code 8).
//   value        (-1)^(code >> 3) * magnitude(code & 7) * 2^(e-127): a bf16 value, exactly.
// Scale bytes 2..252 are valid (a foreign quantiser's too); NaN / Inf weights are outside the rule.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FP4_HD __host__ __device__ inline
#else
#define FP4_HD inline
#endif

namespace fp4 {

constexpr int BLOCK = 32;        // k elements per scale byte
constexpr int SCALE_MIN = 2;     // smallest scale byte the quantiser writes
constexpr int SCALE_MAX = 252;   // largest (E = 254)

FP4_HD uint32_t f32_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
FP4_HD float bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }

// 2^(e-127) for a scale byte e in [1, 254]
FP4_HD float scale_value(unsigned e) { return bits_f32((uint32_t)e << 23); }

// scale byte of a block whose largest |wf| is `amax` (>= 0, finite)
FP4_HD unsigned scale_byte(float amax) {
  const int E = (int)((f32_bits(amax) >> 23) & 0xffu);
  return (unsigned)(E - 2 < SCALE_MIN ? SCALE_MIN : E - 2);
}

// e2m1 code of `wf` under scale byte `e` (2..252)
FP4_HD unsigned code(float wf, unsigned e) {
  const uint32_t b = f32_bits(wf);
  // |wf| * 2^(127-e): a power-of-two factor, exact (an underflow can only happen far below 0.25)
  const float y = bits_f32(b & 0x7fffffffu) * bits_f32((uint32_t)(254u - e) << 23);
  const unsigned mag = (unsigned)(y > 0.25f) + (unsigned)(y >= 0.75f) + (unsigned)(y > 1.25f) + (unsigned)(y >= 1.75f) +
                       (unsigned)(y > 2.5f) + (unsigned)(y >= 3.5f) + (unsigned)(y > 5.0f);
  return ((b >> 31) << 3) | mag;
}

// twice the e2m1 magnitude of a code: {0, 1, 2, 3, 4, 6, 8, 12}
FP4_HD int magnitude2(unsigned c) {
  const int m = (int)(c & 7u);
  return m < 2 ? m : (2 + (m & 1)) << ((m >> 1) - 1);
}

// value of a code under scale byte `e`: sign * magnitude * 2^(e-127)
FP4_HD float value(unsigned c, unsigned e) {
  const float v = 0.5f * (float)magnitude2(c) * scale_value(e);
  return (c & 8u) ? -v : v;
}

}  // namespace fp4
