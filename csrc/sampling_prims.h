// The sampler's workgroup primitives (csrc/sampling.hip), none of which knows about rows, chunks or
// the workspace: the counter-based Gumbel noise, (value, index) maxima, wave reductions on DPP lane
// permutes and the workgroup reductions built on them, order keys, the k-th largest key of an LDS
// array and the first crossing of a histogram prefix. All for workgroups of NT threads.
#pragma once
#include "common.h"

namespace smp {
constexpr int NT = 512;     // threads per workgroup
constexpr int NWV = NT / 64;
constexpr int NB = 2048;    // bins of the decider's histograms
constexpr int NO_TOKEN = 0x7fffffff;     // the index of an ArgMax that has merged nothing

RT_DEVICE uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
RT_DEVICE float gumbel(uint64_t key, uint32_t i) {
  const uint64_t z = mix64((uint64_t)i + key);
  const float u = ((float)(uint32_t)(z >> 40) + 0.5f) * (1.0f / 16777216.0f);
  return -__logf(-__logf(u));
}

struct ArgMax {
  float v;
  int i;
};
RT_DEVICE void am_merge(ArgMax& a, float v, int i) {
  if (v > a.v || (v == a.v && i < a.i)) {
    a.v = v;
    a.i = i;
  }
}
// Wave reductions on DPP lane permutes (VALU, a few cycles each) instead of ds_bpermute shuffles
// (an LDS round trip each): xor 1 and xor 2 as quad permutes, then the half-row and row mirrors
// pair the quads and the 8-lane halves (every lane of a 16-lane row then holds the row's
// result), and the four rows are read out with readlane (wave-uniform result). Fixed pairing
// order: deterministic.
constexpr int DPP_QUAD_1032 = 0xB1, DPP_QUAD_2301 = 0x4E, DPP_ROW_HALF_MIRROR = 0x141, DPP_ROW_MIRROR = 0x140;
template <int CTRL>
RT_DEVICE float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
RT_DEVICE int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
RT_DEVICE float rl(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
RT_DEVICE float wave_sum_dpp(float v) {
  v += dpp_f<DPP_QUAD_1032>(v);
  v += dpp_f<DPP_QUAD_2301>(v);
  v += dpp_f<DPP_ROW_HALF_MIRROR>(v);
  v += dpp_f<DPP_ROW_MIRROR>(v);
  return (rl(v, 0) + rl(v, 16)) + (rl(v, 32) + rl(v, 48));
}
RT_DEVICE float wave_max_dpp(float v) {
  v = fmaxf(v, dpp_f<DPP_QUAD_1032>(v));
  v = fmaxf(v, dpp_f<DPP_QUAD_2301>(v));
  v = fmaxf(v, dpp_f<DPP_ROW_HALF_MIRROR>(v));
  v = fmaxf(v, dpp_f<DPP_ROW_MIRROR>(v));
  return fmaxf(fmaxf(rl(v, 0), rl(v, 16)), fmaxf(rl(v, 32), rl(v, 48)));
}
RT_DEVICE ArgMax wave_argmax_dpp(ArgMax a) {
  am_merge(a, dpp_f<DPP_QUAD_1032>(a.v), dpp_i<DPP_QUAD_1032>(a.i));
  am_merge(a, dpp_f<DPP_QUAD_2301>(a.v), dpp_i<DPP_QUAD_2301>(a.i));
  am_merge(a, dpp_f<DPP_ROW_HALF_MIRROR>(a.v), dpp_i<DPP_ROW_HALF_MIRROR>(a.i));
  am_merge(a, dpp_f<DPP_ROW_MIRROR>(a.v), dpp_i<DPP_ROW_MIRROR>(a.i));
  ArgMax r{rl(a.v, 0), __builtin_amdgcn_readlane(a.i, 0)};
#pragma unroll
  for (int q = 16; q < 64; q += 16) am_merge(r, rl(a.v, q), __builtin_amdgcn_readlane(a.i, q));
  return r;
}
// block reductions: one value per wave through LDS, then every thread folds the NWV values in
// wave order (no second shuffle level)
struct Sum {
  static RT_DEVICE float identity() { return 0.f; }
  static RT_DEVICE float wave(float v) { return wave_sum_dpp(v); }
  static RT_DEVICE float fold(float a, float b) { return a + b; }
};
struct Max {
  static RT_DEVICE float identity() { return -INFINITY; }
  static RT_DEVICE float wave(float v) { return wave_max_dpp(v); }
  static RT_DEVICE float fold(float a, float b) { return fmaxf(a, b); }
};
template <typename Op>
RT_DEVICE float block_reduce(float v, float* scr) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  v = Op::wave(v);
  __syncthreads();
  if (lane == 0) scr[wid] = v;
  __syncthreads();
  float t = Op::identity();
#pragma unroll
  for (int w = 0; w < NWV; ++w) t = Op::fold(t, scr[w]);
  return t;
}
RT_DEVICE ArgMax block_argmax(ArgMax a, float* sv, int* si) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  a = wave_argmax_dpp(a);
  __syncthreads();
  if (lane == 0) {
    sv[wid] = a.v;
    si[wid] = a.i;
  }
  __syncthreads();
  ArgMax b{sv[0], si[0]};
#pragma unroll
  for (int w = 1; w < NWV; ++w) am_merge(b, sv[w], si[w]);
  return b;
}

// order-preserving unsigned key of a float (larger value -> larger key; -inf > 0 = "no entry").
// lo = 16 for bf16 rows: the key's low half carries no order and is cleared, so equal values have
// equal keys whatever their sign (a negative value's ~u would otherwise set the low half to 0xFFFF
// and every tie at a threshold t with a clear low half would compare ABOVE t)
RT_DEVICE uint32_t okey(float v, int lo) {
  const uint32_t u = __float_as_uint(v);
  return ((u & 0x80000000u) ? ~u : (u | 0x80000000u)) & ~((1u << lo) - 1u);
}
RT_DEVICE float okey_value(uint32_t k, int lo) {
  return __uint_as_float(((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k) & ~((1u << lo) - 1u));
}

// The largest t with #{i < n : keys[i] >= t} >= need (the need-th largest key; need <= n), two
// bits per step, down to bit lo (16 for bf16 values: their keys' low half carries no order).
// Counts are wave ballots (a compare + a scalar popcount per key, no shuffles), one barrier per
// step (scr: 2 x 3 x NWV ints, alternating so a step never overwrites what a slower wave reads).
RT_DEVICE uint32_t kth_key(const uint32_t* keys, int n, int need, int lo, int* scr) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t t = 0;
  int par = 0;
  for (int bit = 30; bit >= lo; bit -= 2, par ^= 1) {
    const uint32_t c1 = t | (1u << bit), c2 = t | (2u << bit), c3 = t | (3u << bit);
    int n1 = 0, n2 = 0, n3 = 0;
    for (int i0 = 0; i0 < n; i0 += 8 * NT) {
      uint32_t kk[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = i0 + (int)threadIdx.x + j * NT;
        kk[j] = i < n ? keys[i] : 0u;     // 0: below every value's key
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        n1 += __popcll(__ballot(kk[j] >= c1));
        n2 += __popcll(__ballot(kk[j] >= c2));
        n3 += __popcll(__ballot(kk[j] >= c3));
      }
    }
    int* sc = scr + par * 3 * NWV;
    if (lane == 0) {
      sc[wid] = n1;
      sc[NWV + wid] = n2;
      sc[2 * NWV + wid] = n3;
    }
    __syncthreads();
    n1 = n2 = n3 = 0;
#pragma unroll
    for (int w = 0; w < NWV; ++w) {
      n1 += sc[w];
      n2 += sc[NWV + w];
      n3 += sc[2 * NWV + w];
    }
    t = n3 >= need ? c3 : (n2 >= need ? c2 : (n1 >= need ? c1 : t));
  }
  __syncthreads();   // the caller may rewrite keys / scr
  return t;
}

// First bin whose inclusive prefix of `a` reaches ta or of `bm` reaches tb (NT threads, NB/NT
// bins each); *pa / *pb = the exclusive prefixes before it. Returns NB when none crosses.
RT_DEVICE int first_crossing(const float* a, const float* bm, float ta, float tb, float* scr, int* res, float* pa,
                             float* pb) {
  constexpr int BPT = NB / NT;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  float la[BPT], lb[BPT], sa = 0.f, sb = 0.f;
#pragma unroll
  for (int j = 0; j < BPT; ++j) {
    la[j] = a[BPT * t + j];
    lb[j] = bm[BPT * t + j];
    sa += la[j];
    sb += lb[j];
  }
  const float ta_own = sa, tb_own = sb;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float xa = __shfl_up(sa, o, 64), xb = __shfl_up(sb, o, 64);
    if (lane >= o) {
      sa += xa;
      sb += xb;
    }
  }
  __syncthreads();
  if (lane == 63) {
    scr[wid] = sa;
    scr[NWV + wid] = sb;
  }
  if (t == 0) *res = NB;
  __syncthreads();
  float ca = 0.f, cb = 0.f;
  for (int w = 0; w < wid; ++w) {
    ca += scr[w];
    cb += scr[NWV + w];
  }
  ca += sa - ta_own;     // exclusive prefix before this thread's first bin
  cb += sb - tb_own;
  int cross = NB;
  float ea = 0.f, eb = 0.f;
#pragma unroll
  for (int j = 0; j < BPT; ++j) {
    if (cross == NB && (ca + la[j] >= ta || cb + lb[j] >= tb)) {
      cross = BPT * t + j;
      ea = ca;
      eb = cb;
    }
    ca += la[j];
    cb += lb[j];
  }
  if (cross < NB) atomicMin(res, cross);
  __syncthreads();
  const int cbin = *res;
  if (cbin < NB && cross == cbin) {
    *pa = ea;
    *pb = eb;
  }
  __syncthreads();
  return cbin;
}
}  // namespace smp
