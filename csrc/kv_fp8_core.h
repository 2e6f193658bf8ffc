// The scalar rule of the FP8 KV cache (kv_dtype "fp8": OCP e4m3fn codes, one byte per K / V
// element, one fp32 k_scale and one v_scale per layer; ops/reference.py kv_fp8_code / kv_fp8_value
// is the contract). __host__ __device__: every cache writer and the host check
// (csrc/tests/kv_fp8_check.cpp) run the same copy.
//
//   encode   code = e4m3fn_rne(clamp(y * inv_scale, +-448)): ONE fp32 multiply, then the convert.
//            y is the fp32 value a writer would otherwise round to bf16. +-inf saturates to +-448,
//            NaN gives the NaN code 0x7f. The sign bit is kept (a negative value that rounds to
//            zero is 0x80).
//   decode   value = e4m3(code) * scale. e4m3 values are bf16 values, so the convert is exact; the
//            attention kernels fold k_scale into the softmax scale and v_scale into the final 1/l
//            normalisation, and the key loop has no scale multiply.
//   zero     byte 0 is +0: a zero-initialised pool holds finite keys and values.
// On the device the convert is v_cvt_pk_fp8_f32 (gfx950: OCP e4m3fn, RNE); the host runs the
// integer statement of the same rounding below, and the two are held together byte for byte by
// tests/test_kv_fp8_gpu.py over every finite bf16 input.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KV8_HD __host__ __device__ inline
#else
#define KV8_HD inline
#endif

namespace kv8 {

constexpr float MAX = 448.f;          // largest finite e4m3fn value
constexpr unsigned NAN_CODE = 0x7fu;

KV8_HD uint32_t f32_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
KV8_HD float bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }

// e4m3fn code of x, |x| <= 448, not NaN: round to nearest, ties to even (integer arithmetic)
KV8_HD unsigned e4m3_rne(float x) {
  const uint32_t b = f32_bits(x);
  const unsigned sign = (b >> 31) << 7;
  const uint32_t a = b & 0x7fffffffu;
  const int e = (int)(a >> 23) - 127;
  if (e < -6) {
    // below the smallest normal 2^-6: multiples of 2^-9 (|x| * 512 is exact, < 8)
    const float f = bits_f32(a) * 512.f;
    unsigned i = (unsigned)f;
    const float frac = f - (float)i;
    if (frac > 0.5f || (frac == 0.5f && (i & 1u))) ++i;
    return sign | i;   // i == 8 is the code of 2^-6
  }
  const uint32_t m = a & 0x7fffffu;
  unsigned r = m >> 20;
  const uint32_t rem = m & 0xfffffu;
  if (rem > 0x80000u || (rem == 0x80000u && (r & 1u))) ++r;
  return sign | ((((unsigned)(e + 7)) << 3) + r);   // a mantissa carry moves into the exponent
}

// the cache byte of the fp32 value y under inv_scale = 1 / scale
KV8_HD unsigned code(float y, float inv_scale) {
  float t = y * inv_scale;
  if (t != t) return NAN_CODE;
  t = t < -MAX ? -MAX : (t > MAX ? MAX : t);
#if defined(__HIP_DEVICE_COMPILE__)
  return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(t, t, 0, false) & 0xffu;
#else
  return e4m3_rne(t);
#endif
}

// e4m3fn value of a code (exact; 0x7f / 0xff: NaN)
KV8_HD float e4m3_value(unsigned c) {
  const unsigned e = (c >> 3) & 15u, m = c & 7u;
  if (e == 15u && m == 7u) return bits_f32(0x7fc00000u);
  const float v = e == 0u ? (float)m * bits_f32((127u - 9u) << 23)
                          : bits_f32(((e + 120u) << 23) | (m << 20));
  return (c & 0x80u) ? -v : v;
}

KV8_HD float value(unsigned c, float scale) { return e4m3_value(c) * scale; }

}  // namespace kv8

// The contract's names (ops/reference.py kv_fp8_code / kv_fp8_value), as the writers call them. The
// host/device marker is this header's own (KV8_HD), as fp4_core.h has FP4_HD: the header stays
// includable without common.h.
KV8_HD unsigned kv_fp8_code(float y, float inv_scale) { return kv8::code(y, inv_scale); }
KV8_HD float kv_fp8_value(unsigned code, float scale) { return kv8::value(code, scale); }
