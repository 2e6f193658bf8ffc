// Host-side launch plan of K3, paged decode attention (attention_decode.hip): the attention grid,
// its kernel variant (GM, loop form, K/V load mode), whether the splits are combined in the launch,
// by the separate combine launch or by the caller, and that combine's geometry — a pure function
// of the shape and the experiment knobs. No HIP calls and no environment reads in
// plan_paged_decode / combine_slot_bound, so csrc/tests/host_check.cpp exercises every rule
// without a GPU.
#pragma once
#include "attn_core.h"

#include <cstdlib>

namespace attn {

// The experiment knobs (tools/microbench.py, profiles/): read from the environment once per
// process by knobs().
struct AttnKnobs {
  int probe = 0;                 // RT_ATTN_PROBE=<k>: latency probe, stop after phase k (attn_item)
  int ext_splits = 2;            // RT_ATTN_EXT_SPLITS: separate combine from this many splits on (0 = never)
  bool skip_combine = false;     // RT_ATTN_SKIP_COMBINE=1: the attention launch without its combine launch
  int pp = -1;                   // RT_ATTN_PP=0 / 1 pins the K/V loop form (-1: the rule)
  int lm = LM_NTK | LM_NTV;      // RT_ATTN_LM: K/V load mode (1 = K nt, 2 = V nt, 3 = both, 7 = LDS-DMA staged)
  int combine_nsl = 32;          // RT_COMBINE_NSL: slot-lane cap of the combine (multiples of 8 in [8, 128])
};
inline const AttnKnobs& knobs() {
  static const AttnKnobs k = [] {
    AttnKnobs k;
    const auto num = [](const char* name, int dflt) {
      const char* e = getenv(name);
      return e ? atoi(e) : dflt;
    };
    k.probe = num("RT_ATTN_PROBE", k.probe);
    k.ext_splits = num("RT_ATTN_EXT_SPLITS", k.ext_splits);
    k.skip_combine = num("RT_ATTN_SKIP_COMBINE", 0) == 1;
    k.pp = num("RT_ATTN_PP", k.pp);
    k.lm = num("RT_ATTN_LM", k.lm);
    k.combine_nsl = num("RT_COMBINE_NSL", k.combine_nsl);
    return k;
  }();
  return k;
}

// Partial slots per query row the combine launch is sized for: every split of every member of
// the largest group a row can be in (n * G <= GROUP_COLS), within the row's stride. The host
// sizes the launch with it and decode_combine_kernel bounds its first loads with it (slots past
// the row's own count are inside the row's stride and loaded, never merged).
RT_HD int combine_slot_bound(bool grouped, int G, int num_splits, int stride) {
  const int all = (GROUP_COLS / G) * num_splits;
  return grouped ? (stride < all ? stride : all) : num_splits;
}

struct AttnPlan {
  int rc = 0;                  // 0, or -1 head ratio, -3 splits > MAXS, -4 group slots < splits,
                               // -5 plan row without ids, -2 head dim (launch_paged_decode adds -6),
                               // -7 fp8 cache with a head dim other than 128
  int splits = 1;              // num_splits, at least 1
  int gx = 0, gy = 0, block = NW * 64;   // attention launch; gx == 0: empty batch, nothing runs
  int GM = GROUP_COLS;         // query columns the workgroup's LDS holds
  bool pp = true;              // ping-pong K/V loop (false: the copy loop)
  int lm = 0;                  // K/V load mode (LM_*)
  bool ext_combine = false;    // partials left for a combine after the launch
  bool deferred = false;       // ... which the caller runs (combine_o.hip: combine + o-projection)
  bool combine = false;        // ... which decode_combine_kernel runs:
  int nmax = 0;                // slots per row it is sized for (combine_slot_bound)
  int nsl = 0, spl = 0;        // slot-lanes per workgroup, slots per lane per chunk (1, 2, 4, 8)
  int cgx = 0, cgy = 0, cblock = 0;
};

inline AttnPlan plan_paged_decode(int B, int Hq, int Hkv, int D, int num_splits, bool grouped, int slot_stride,
                                  bool has_plan, int plan_stride, bool defer_combine, const AttnKnobs& kn,
                                  bool kv_fp8 = false) {
  AttnPlan pl;
  if (B == 0) return pl;
  pl.splits = num_splits < 1 ? 1 : num_splits;
  pl.rc = Hq % Hkv || Hq / Hkv > GROUP_COLS          ? -1   // the first that applies, in this order
          : pl.splits > MAXS                         ? -3
          : grouped && slot_stride < pl.splits       ? -4
          : has_plan && plan_stride <= PLAN_HDR      ? -5
          : D != 128 && D != 64                      ? -2
          : kv_fp8 && D != 128                       ? -7   // fp8 caches: D = 128 only
                                                     : 0;
  if (pl.rc != 0) return pl;
  const int G = Hq / Hkv;
  pl.gx = B * Hkv;
  pl.gy = pl.splits;
  // GM = 4 (Llama-3-8B, Mistral-7B, no groups) keeps the workgroup at ~26 KB of LDS so two fit a
  // CU; a group's n * G columns need the 16-column merge buffers.
  // (16-wave grouped workgroups were measured and rejected: __launch_bounds__(1024) caps the item
  // at 128 VGPRs, it spills, and half the CUs stream — 22K shared keys 25.0 -> 41.6 us at 6 splits,
  // profiles/r06/attn_kchunk.md)
  pl.GM = grouped ? GROUP_COLS : (G <= 4 ? 4 : (G <= 8 ? 8 : 16));
  // K/V loop form (attn_core.h PP): the copy-free ping-pong wins where a workgroup streams many
  // tiles (Llama-3-8B tp 1, 8 KV heads: 3 knights x 22K shared keys 29.6 -> 28.7 us, 40K 41.1 ->
  // 40.8 us) and loses ~0.3 us on the short ranges of 1-2 KV-head shards (tp 4 / 8), which keep the
  // copy loop (profiles/r05/attn_pingpong_ab.md). RT_ATTN_PP=0 / 1 pins it (A/B).
  pl.pp = kn.pp >= 0 ? kn.pp != 0 : Hkv >= 4;
  // K/V load mode (attn_core.h LM_*): nontemporal K and V loads. With the chunk-major K blocks,
  // tp 1, 3 knights x 22K / 40K shared keys 27.6 -> 25.4 / 41.9 -> 37.8 us; rows with distinct
  // contexts B = 1 25K 25.9 -> 23.7, B = 3 25K 59.3 -> 55.3, B = 16 2K 31.0 -> 28.6; tp 8 shard even
  // (profiles/r06/attn_kchunk.md). The one loser: ungrouped rows that read the SAME blocks (3 rows
  // over one 22K prefix without groups, 33.5 -> 35.4: the 2nd / 3rd reads no longer hit L2 / MALL)
  // — the engine decodes shared prefixes as groups, so that case does not arise there.
  // RT_ATTN_LM pins the mode (A/B; 7 = both through the LDS-DMA staged loop, ping-pong form only).
  // An fp8 cache has the register forms only: RT_ATTN_LM=7 falls back to its two nt bits.
  pl.lm = (kn.lm & LM_GLDS) && pl.pp && !kv_fp8 ? 7 : kn.lm & 3;
  // separate combine launch from this many splits on (RT_ATTN_EXT_SPLITS pins it; 0 = never):
  // r03 probes, 3 knights x 40K shared keys: in-launch combine 8.7 us at 16 splits (48 slots),
  // 23 us at 64 (192 slots); whole launch(es), grouped B=3: tp8 shard 32.6 -> 14.9 us (64
  // splits), tp1 41.0 -> 38.7 us (8 splits) — the extra boundary costs less than the serial
  // combine on one CU at every measured split count (profiles/r03/attn_ext_combine.md)
  pl.ext_combine = kn.ext_splits > 0 && pl.splits >= kn.ext_splits && kn.probe == 0;
  // (never with an fp8 cache: the caller's combine does not know the V scale)
  pl.deferred = pl.ext_combine && defer_combine && D == 128 && !kv_fp8;
  pl.combine = pl.ext_combine && !pl.deferred && !kn.skip_combine;
  if (!pl.combine) return pl;
  pl.nmax = combine_slot_bound(grouped, G, pl.splits, slot_stride);
  // slot-lanes (x 8 dim-lanes) per workgroup, capped at 32 (RT_COMBINE_NSL): fewer, wider lanes
  // (8 slots each for a tp 8 table's 256-slot bound) beat 128 lanes x 2 — 4 waves to dispatch
  // and merge instead of 16; tp 8 grouped attention + combine 12.4 -> 11.6 us
  // (profiles/r04/combine_lanes_ab.md)
  const int cap = kn.combine_nsl >= 8 && kn.combine_nsl <= 128 && kn.combine_nsl % 8 == 0 ? kn.combine_nsl : 32;
  const int want = (pl.nmax + 7) / 8 * 8;
  pl.nsl = cap < want ? cap : want;
  const int per = (pl.nmax + pl.nsl - 1) / pl.nsl;
  pl.spl = per <= 1 ? 1 : (per <= 2 ? 2 : (per <= 4 ? 4 : 8));
  if ((pl.nmax + pl.spl - 1) / pl.spl < pl.nsl) pl.nsl = ((pl.nmax + pl.spl - 1) / pl.spl + 7) / 8 * 8;
  pl.cgx = B * Hq;
  pl.cgy = D / 32;
  pl.cblock = 8 * pl.nsl;
  return pl;
}

}  // namespace attn
