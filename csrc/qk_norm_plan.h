// Launch plan of the QK-norm + RoPE + paged K/V write kernel (csrc/qk_norm_rope.hip): one pure host
// function, run by the launcher before any HIP call and by csrc/tests/qk_norm_check.cpp.
//
// Work: one wave per (token, head slot), Hq + 2 Hkv head slots per token, WAVES waves per workgroup.
//   >= 0  the grid (0: nothing to launch, T == 0)
//   -1    a shape, scale or eps the kernel does not take, or a missing operand
//   -2    more waves than a 32-bit index holds
#pragma once
#include <cmath>
#include <cstdint>

namespace qkn {

constexpr int WAVES = 4;            // waves per workgroup
constexpr int THREADS = WAVES * 64;

// ``kv8``: the caches hold e4m3fn bytes (kv_dtype "fp8"); ``k_scale`` / ``v_scale`` are checked either
// way (a bf16 launch passes 1). ``operands``: every pointer the launch reads is there (the cos|sin
// table included when it rotates).
inline int plan(int64_t T, int Hq, int Hkv, int D, int BS, bool kv8, float k_scale, float v_scale, float eps,
                bool operands = true) {
  if (T < 0 || Hq < 1 || Hkv < 1 || BS < 1) return -1;
  if (D != 64 && D != 128) return -1;                        // lane l holds dims l and l + D/2 of one head
  if (kv8 && (D % 64 || BS % 8)) return -1;                  // the fp8 block layouts (common.h kc8_elem / vc8_elem)
  if (!(k_scale > 0.f) || !(v_scale > 0.f) || !(k_scale <= 3.0e38f) || !(v_scale <= 3.0e38f)) return -1;
  if (!std::isfinite(eps) || eps < 0.f) return -1;
  const int64_t waves = T * ((int64_t)Hq + 2 * (int64_t)Hkv);
  if (waves > (int64_t)INT32_MAX) return -2;
  if (T == 0) return 0;
  if (!operands) return -1;
  return (int)((waves + WAVES - 1) / WAVES);
}

}  // namespace qkn
