// K3: paged-KV decode attention (one query token per sequence), GQA, MFMA bf16, split-KV.
// What lives where:
//   attn_core.h  the device core (shared with the persistent decode-layer experiment): the work
//                item attn_item, and the rules with one copy each — item_range (an item's keys),
//                group_record (a row's effective group), merge_state (two softmax states);
//   attn_plan.h  the pure host plan: knobs, grids, kernel variant, which combine runs and its
//                geometry (combine_slot_bound), tested without a GPU by csrc/tests/host_check.cpp;
//   this file    the three kernels around the core — attention (blockIdx = (sequence x kv head,
//                key split)), the per-step work plan, the separate split combine — and the
//                launchers: validate -> plan -> fill AttnArgs -> dispatch.
#include "attn_plan.h"

#include <type_traits>

namespace {
using namespace attn;

// the LDS-DMA staged form (LM_GLDS) puts each wave's K/V slice over the merge buffers
template <int D, int GM, int W, int LM>
union DecodeSmem {
  AttnSmem<D, GM, W> m;
  short8 stage[(LM & LM_GLDS) ? W * tile_words<D>() * 64 : 1];
};

template <int D, int GM, int W = NW, bool PP = true, int LM = 0>
__global__ void __launch_bounds__(W * 64) paged_decode_kernel(AttnArgs p) {
  static_assert(sizeof(DecodeSmem<D, GM, W, LM>) <= 160 * 1024, "LDS of one CU");
  __shared__ DecodeSmem<D, GM, W, LM> sm_;
  attn_item<D, false, GM, W, PP, LM>(p, blockIdx.x, blockIdx.y, sm_.m);
}

// The same over an fp8 (e4m3fn) K/V cache: attn_core.h Tile8 (half the tile registers, converted
// to bf16 fragments in `step`), k_scale inside scale_log2, v_scale where O is normalised.
template <int D, int GM, bool PP, int LM>
__global__ void __launch_bounds__(NW * 64) paged_decode_fp8_kernel(AttnArgs p) {
  __shared__ AttnSmem<D, GM, NW> sm_;
  attn_item<D, false, GM, NW, PP, LM, true>(p, blockIdx.x, blockIdx.y, sm_);
}

// Per-step work plan: one workgroup per item (sequence b, split) writes the item's key range
// (item_range, exactly as attn_item derives it) and its block ids. A decode step runs this once;
// every layer's attention launch then requests an item header and its first block ids together
// at launch-known addresses — one dependent round trip ahead of the K/V stream instead of two.
__global__ void __launch_bounds__(256) attn_plan_kernel(AttnArgs p, int G, int GM, int* __restrict__ plan) {
  const int b = blockIdx.x, split = blockIdx.y;
  const bool grouped = p.groups != nullptr;
  const int* gp = grouped ? p.groups + 3 * b : p.ctx_lens + b;
  const int go = grouped ? 1 : 0;
  const ItemRange it = item_range(p.ctx_lens[b], gp[0], gp[go], gp[2 * go], grouped, b, split, G, GM, p.num_splits);
  int* hdr = plan + (size_t)(b * p.num_splits + split) * p.plan_stride;
  if (threadIdx.x == 0) {
    hdr[0] = it.b0; hdr[1] = it.n; hdr[2] = it.sh; hdr[3] = it.ctx;
    hdr[4] = it.sh_b; hdr[5] = it.nsh; hdr[6] = it.pr_b; hdr[7] = it.nv;
  }
  const int lim = min(it.nv, p.plan_stride - PLAN_HDR);
  for (int tt = threadIdx.x; tt < lim; tt += blockDim.x)
    hdr[PLAN_HDR + tt] = tt < it.nsh ? p.block_tables[(size_t)it.b0 * p.max_blocks + it.sh_b + tt]
                                     : p.block_tables[(size_t)b * p.max_blocks + it.pr_b + (tt - it.nsh)];
}

// Split-KV combine as its own launch, for launches with many partial slots per query row
// (tensor-parallel shards: 1-2 KV heads per rank -> 32-64 splits so the K/V stream still
// covers the CUs; a table of 3 knights then leaves 3 x 64 = 192 slots per row). The in-launch
// combine runs on the ONE last-arriving workgroup, whose CU reads every partial of the row
// (cross-XCD hand-off reads ~65 GB/s per CU, MI355X_MICROARCH handoff-payload): 23 us for 192
// slots at 4 query heads (r03 probe). Here every (row, 32-dim chunk) gets its own workgroup of
// 8 dim-lanes x NSL slot-lanes (NSL = blockDim / 8, sized by the host to the row's slots, <= 128),
// each lane owning SPL slots whose loads are ALL issued before the first merge: one round trip
// per launch instead of one per 32 slots (round 3: 6 dependent trips at 192 slots, 6.6 us), and
// that trip overlaps the group-record lookup (the host's slot bound needs no record).
// Merge order is fixed (lane-local slots in index order, then xor-shuffle pairs, then a tree
// over the waves through LDS), so the result does not depend on timing.
// Partials were stored write-through by the previous launch: the kernel boundary orders them.
// KV8: the partials came from an fp8 cache, the final rows take the V scale (AttnArgs::v_scale).
template <int D, int SPL, bool KV8 = false>
__global__ void __launch_bounds__(1024) decode_combine_kernel(AttnArgs p) {
  const int G = p.Hq / p.Hkv;
  const int row = blockIdx.x;                  // b * Hq + query head
  const int chunk = blockIdx.y;
  const int b = row / p.Hq;
  const int dl = threadIdx.x & 7, sl = threadIdx.x >> 3;
  const int nsl = blockDim.x >> 3;
  const int d0 = chunk * 32 + 4 * dl;
  const int stride = p.slot_stride > 0 ? p.slot_stride : p.num_splits;
  const int nmax = combine_slot_bound(p.groups != nullptr, G, p.num_splits, stride);   // the host's sizing
  const float* __restrict__ po = p.part_o + (size_t)row * stride * D;
  const float* __restrict__ pml = p.part_ml + (size_t)row * stride * 4;
  // the group record and the first chunk's partials are independent: both requests go out
  // before either is used, the vector loads first (the compiler waits for a conditional block's
  // scalar loads at its end; round 3 paid the group lookup as a trip ahead of the partials)
  float4_ mlv[SPL], ov[SPL];
#pragma unroll
  for (int j = 0; j < SPL; ++j) {
    const int s = min(sl + j * nsl, nmax - 1);
    mlv[j] = *reinterpret_cast<const float4_*>(pml + (size_t)s * 4);
    ov[j] = *reinterpret_cast<const float4_*>(po + (size_t)s * D + d0);
  }
  int b0 = 0, nn = 1, sh = 0;
  if (p.groups != nullptr) {
    b0 = p.groups[3 * b];
    nn = p.groups[3 * b + 1];
    sh = p.groups[3 * b + 2];
  }
  const int nslots = group_record(p.groups != nullptr, b0, nn, sh, b, G).n * p.num_splits;
  if (nslots == 1) return;                     // written directly by the attention launch
  float M = -INFINITY, L = 0.f;
  float4_ O = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < SPL; ++j)
    if (sl + j * nsl < nslots) merge_state(M, L, O, mlv[j][0], mlv[j][1], ov[j]);
  // more chunks only for rows with more slots than the host sized for (not reached when the
  // group record is well-formed: n * G <= 16)
  for (int base = SPL * nsl; base < nslots; base += SPL * nsl) {
#pragma unroll
    for (int j = 0; j < SPL; ++j) {            // every load of the chunk in flight before any merge
      const int s = min(base + sl + j * nsl, nslots - 1);
      mlv[j] = *reinterpret_cast<const float4_*>(pml + (size_t)s * 4);
      ov[j] = *reinterpret_cast<const float4_*>(po + (size_t)s * D + d0);
    }
#pragma unroll
    for (int j = 0; j < SPL; ++j)
      if (base + sl + j * nsl < nslots) merge_state(M, L, O, mlv[j][0], mlv[j][1], ov[j]);
  }
  // the 8 slot-lanes of a wave (lane bits 3..5), then the waves through LDS; fixed order
  auto xmerge = [&](int x, bool upper) {
    const float m2 = __shfl_xor(M, x, 64), l2 = __shfl_xor(L, x, 64);
    float4_ o2;
#pragma unroll
    for (int i = 0; i < 4; ++i) o2[i] = __shfl_xor(O[i], x, 64);
    if (upper) {   // the upper partner takes the lower's state first: same order on both
      const float mm = M, ll = L;
      const float4_ oo = O;
      M = m2; L = l2; O = o2;
      merge_state(M, L, O, mm, ll, oo);
    } else {
      merge_state(M, L, O, m2, l2, o2);
    }
  };
#pragma unroll
  for (int x = 8; x < 64; x <<= 1) xmerge(x, sl & (x >> 3));
  __shared__ float red[16][8][6];
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  if ((threadIdx.x & 63) < 8) {
    float* e = red[wave][dl];
    e[0] = O[0]; e[1] = O[1]; e[2] = O[2]; e[3] = O[3]; e[4] = M; e[5] = L;
  }
  __syncthreads();
  // the waves' states as a tree on the first wave: lane (w, dl) of 8 groups takes waves w and
  // w + 8, then three xor steps — 4 dependent merges instead of nwaves - 1
  if (threadIdx.x < 64) {
    const int w = threadIdx.x >> 3;
    M = -INFINITY; L = 0.f; O = float4_{0.f, 0.f, 0.f, 0.f};
    if (w < nwaves) {
      const float* e = red[w][dl];
      merge_state(M, L, O, e[4], e[5], float4_{e[0], e[1], e[2], e[3]});
    }
    if (w + 8 < nwaves) {
      const float* e = red[w + 8][dl];
      merge_state(M, L, O, e[4], e[5], float4_{e[0], e[1], e[2], e[3]});
    }
#pragma unroll
    for (int x = 8; x < 64; x <<= 1) xmerge(x, w & (x >> 3));
    if (w == 0) {
      float inv = L > 0.f ? 1.f / L : 0.f;
      if constexpr (KV8) inv *= p.v_scale;
      store_bf16x4(p.out + (size_t)row * D + d0, O[0] * inv, O[1] * inv, O[2] * inv, O[3] * inv, false);
    }
  }
}

// Runtime value -> compile-time constant: f(integral_constant<int, V>) for the V that equals v;
// -2 if none does (the plan has refused such values before a dispatch sees them).
template <int... Vs, class F>
int with_const(int v, F&& f) {
  int rc = -2;
  ((v == Vs ? void(rc = f(std::integral_constant<int, Vs>{})) : void()), ...);
  return rc;
}

int launch(void (*kernel)(AttnArgs), dim3 grid, dim3 block, hipStream_t stream, const AttnArgs& args) {
  hipLaunchKernelGGL(kernel, grid, block, 0, stream, args);
  return hipGetLastError() == hipSuccess ? 0 : -6;
}
}  // namespace

// The limits the Python side repeats (ops/__init__.py), exported so a test holds them together
int attn_plan_hdr() { return PLAN_HDR; }
int attn_max_splits() { return MAXS; }
int attn_group_cols() { return GROUP_COLS; }

// q [B, Hq, D]; k_cache [NB, Hkv, 32, D] (chunk-major blocks, common.h kc_elem); v_cache [NB, Hkv, D, 32]; block_tables [B, max_blocks] int32;
// defer_combine: leave the separate combine to the caller (*deferred = 1 when it was needed);
// part_o >= B*Hq*slot_stride*D floats, part_ml >= B*Hq*slot_stride*4 floats, counters >= B*Hkv ints
// (zeroed once). groups: nullptr or [B][3] {first, n, shared blocks} (shared-prefix groups,
// attn_core.h); slot_stride >= max n * num_splits (0 = num_splits, no groups).
// Returns 0, the plan's refusal (attn_plan.h AttnPlan::rc: -1 .. -5) or -6: a launch failed.
static int decode_launch(void* out, const void* q, const void* k_cache, const void* v_cache, const int* block_tables,
                         const int* ctx_lens, float* part_o, float* part_ml, int* counters, int B, int Hq, int Hkv,
                         int D, int max_blocks, float scale, int num_splits, const int* groups, int slot_stride,
                         hipStream_t stream, int defer_combine, int* deferred, const int* plan, int plan_stride,
                         bool kv_fp8, float k_scale, float v_scale) {
  if (deferred != nullptr) *deferred = 0;
  const AttnKnobs& kn = knobs();
  const AttnPlan pl = plan_paged_decode(B, Hq, Hkv, D, num_splits, groups != nullptr, slot_stride, plan != nullptr,
                                        plan_stride, defer_combine != 0, kn, kv_fp8);
  if (pl.rc != 0 || pl.gx == 0) return pl.rc;
  AttnArgs args{(uint16_t*)out, (const uint16_t*)q, (const uint16_t*)k_cache, (const uint16_t*)v_cache,
                block_tables, ctx_lens, part_o, part_ml, counters, Hq, Hkv, max_blocks, scale * LOG2E, pl.splits,
                groups, groups != nullptr ? slot_stride : 0};
  args.probe = kn.probe;
  args.ext_combine = pl.ext_combine ? 1 : 0;
  args.plan = plan;
  args.plan_stride = plan != nullptr ? plan_stride : 0;
  if (kv_fp8) {
    // value = e4m3(code) * scale: k_scale joins the softmax scale, v_scale the final normalisation
    args.scale_log2 = scale * k_scale * LOG2E;
    args.v_scale = v_scale;
    int rc8 = with_const<4, 8, 16>(pl.GM, [&](auto gm) {
      return with_const<1, 0>(pl.pp, [&](auto pp) {
        return with_const<0, 1, 2, 3>(pl.lm, [&](auto lm) {
          return launch(paged_decode_fp8_kernel<128, gm(), pp() != 0, lm()>, dim3(pl.gx, pl.gy), dim3(pl.block),
                        stream, args);
        });
      });
    });
    if (rc8 != 0 || !pl.combine) return rc8;
    return with_const<1, 2, 4, 8>(pl.spl, [&](auto spl) {
      return launch(decode_combine_kernel<128, spl(), true>, dim3(pl.cgx, pl.cgy), dim3(pl.cblock), stream, args);
    });
  }
  int rc = with_const<128, 64>(D, [&](auto d) {
    return with_const<4, 8, 16>(pl.GM, [&](auto gm) {
      return with_const<1, 0>(pl.pp, [&](auto pp) {
        return with_const<0, 1, 2, 3, 7>(pl.lm, [&](auto lm) {
          return launch(paged_decode_kernel<d(), gm(), NW, pp() != 0, lm()>, dim3(pl.gx, pl.gy), dim3(pl.block),
                        stream, args);
        });
      });
    });
  });
  if (rc != 0) return rc;
  if (pl.deferred && deferred != nullptr) *deferred = 1;
  if (!pl.combine) return 0;
  return with_const<128, 64>(D, [&](auto d) {
    return with_const<1, 2, 4, 8>(pl.spl, [&](auto spl) {
      return launch(decode_combine_kernel<d(), spl()>, dim3(pl.cgx, pl.cgy), dim3(pl.cblock), stream, args);
    });
  });
}

int launch_paged_decode(void* out, const void* q, const void* k_cache, const void* v_cache, const int* block_tables,
                        const int* ctx_lens, float* part_o, float* part_ml, int* counters, int B, int Hq, int Hkv,
                        int D, int max_blocks, float scale, int num_splits, const int* groups, int slot_stride,
                        hipStream_t stream, int defer_combine, int* deferred, const int* plan, int plan_stride) {
  return decode_launch(out, q, k_cache, v_cache, block_tables, ctx_lens, part_o, part_ml, counters, B, Hq, Hkv, D,
                       max_blocks, scale, num_splits, groups, slot_stride, stream, defer_combine, deferred, plan,
                       plan_stride, false, 1.f, 1.f);
}

// The same over an fp8 K/V cache (e4m3fn bytes in the layouts of common.h kc8_elem / vc8_elem, same
// tensor shapes; k_scale / v_scale: value = e4m3(code) * scale). D = 128 only (-7 otherwise); a
// scale that is not finite and > 0 is -8, before any HIP call. The combine is never deferred.
int launch_paged_decode_fp8(void* out, const void* q, const void* k_cache, const void* v_cache,
                            const int* block_tables, const int* ctx_lens, float* part_o, float* part_ml,
                            int* counters, int B, int Hq, int Hkv, int D, int max_blocks, float scale, int num_splits,
                            const int* groups, int slot_stride, hipStream_t stream, const int* plan, int plan_stride,
                            float k_scale, float v_scale) {
  if (!(k_scale > 0.f) || !(v_scale > 0.f) || !(k_scale <= 3.0e38f) || !(v_scale <= 3.0e38f)) return -8;
  return decode_launch(out, q, k_cache, v_cache, block_tables, ctx_lens, part_o, part_ml, counters, B, Hq, Hkv, D,
                       max_blocks, scale, num_splits, groups, slot_stride, stream, 0, nullptr, plan, plan_stride, true,
                       k_scale, v_scale);
}

// The per-step plan for launch_paged_decode's ``plan`` (same B, heads, num_splits, groups, block
// tables and lengths as the launches that read it): plan >= B * num_splits * plan_stride ints.
int launch_attn_plan(int* plan, int plan_stride, const int* block_tables, const int* ctx_lens, const int* groups,
                     int B, int Hq, int Hkv, int max_blocks, int num_splits, hipStream_t stream) {
  if (B == 0) return 0;
  if (Hq % Hkv || Hq / Hkv > GROUP_COLS || num_splits < 1 || num_splits > MAXS || plan_stride <= PLAN_HDR) return -1;
  AttnArgs args{};
  args.block_tables = block_tables;
  args.ctx_lens = ctx_lens;
  args.max_blocks = max_blocks;
  args.num_splits = num_splits;
  args.groups = groups;
  args.plan_stride = plan_stride;
  hipLaunchKernelGGL(attn_plan_kernel, dim3(B, num_splits), dim3(256), 0, stream, args, Hq / Hkv, GROUP_COLS, plan);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}
