"""Op dispatch: hand-written HIP/CDNA4 kernels on GPU tensors, PyTorch reference on CPU.

GPU tensors ALWAYS go to the native extension ``theroundtaible_amd._C`` (built
in-tree by ``csrc/build.py``); if it is missing on a GPU box the op raises instead
of silently falling back, so a test can never pass on eager PyTorch while claiming
to exercise the kernels. (``ROUNDTABLE_ALLOW_TORCH_FALLBACK=1`` exists only for
debugging a broken build.)
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from . import reference as ref

_NATIVE = None
_NATIVE_ERR: Optional[BaseException] = None


def native():
    """The compiled extension module (raises if it cannot be imported)."""
    global _NATIVE, _NATIVE_ERR
    if _NATIVE is None and _NATIVE_ERR is None:
        try:
            from .. import _C  # type: ignore
            _NATIVE = _C
        except BaseException as e:  # noqa: BLE001
            _NATIVE_ERR = e
    if _NATIVE is None:
        raise RuntimeError(f"theroundtaible_amd._C (HIP kernels) is not built/importable: {_NATIVE_ERR}. "
                           f"Run `python csrc/build.py` (or __graft_entry__.build()).")
    return _NATIVE


def native_available() -> bool:
    try:
        native()
        return True
    except RuntimeError:
        return False


def _use_native(t: torch.Tensor) -> bool:
    if not t.is_cuda:
        return False
    if os.environ.get("ROUNDTABLE_ALLOW_TORCH_FALLBACK") == "1" and not native_available():
        return False
    return True


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    if _use_native(x):
        out = torch.empty_like(x)
        native().rms_norm(out, x, w, eps)
        return out
    return ref.rms_norm(x, w, eps)


def fused_add_rms_norm(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor,
                       eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """Returns (rmsnorm(x + residual), x + residual). On GPU ``residual`` is updated in place."""
    if _use_native(x):
        out = torch.empty_like(x)
        native().fused_add_rms_norm(out, x, residual, w, eps)
        return out, residual
    return ref.fused_add_rms_norm(x, residual, w, eps)


def layer_norm(x, w, b, eps):
    if _use_native(x):
        out = torch.empty_like(x)
        native().layer_norm(out, x, w, b, eps)
        return out
    return ref.layer_norm(x, w, b, eps)


def fused_add_layer_norm(x, residual, w, b, eps):
    if _use_native(x):
        out = torch.empty_like(x)
        native().fused_add_layer_norm(out, x, residual, w, b, eps)
        return out, residual
    return ref.fused_add_layer_norm(x, residual, w, b, eps)


def rope_and_cache(qkv: torch.Tensor, positions: torch.Tensor, cos_sin: Optional[torch.Tensor],
                   k_cache: torch.Tensor, v_cache: torch.Tensor, slot_mapping: torch.Tensor,
                   n_heads: int, n_kv_heads: int, head_dim: int, k_scale: float = 1.0,
                   v_scale: float = 1.0) -> torch.Tensor:
    """``k_scale`` / ``v_scale``: read only with an fp8 cache (uint8 tensors of the same shapes, kv_dtype
    "fp8"): the cache then takes ``kv_fp8_code(value, 1 / scale)`` bytes (ops/reference.py)."""
    if _use_native(qkv):
        q = torch.empty(qkv.shape[0], n_heads, head_dim, dtype=qkv.dtype, device=qkv.device)
        cs = cos_sin if cos_sin is not None else torch.empty(0, device=qkv.device)
        if ref.is_fp8_cache(k_cache, v_cache):
            native().rope_and_cache_fp8(q, qkv, positions, cs, k_cache, v_cache, slot_mapping, n_heads, n_kv_heads,
                                        head_dim, float(k_scale), float(v_scale))
        else:
            native().rope_and_cache(q, qkv, positions, cs, k_cache, v_cache, slot_mapping, n_heads, n_kv_heads,
                                    head_dim)
        return q
    return ref.rope_and_cache(qkv, positions, cos_sin, k_cache, v_cache, slot_mapping, n_heads, n_kv_heads, head_dim,
                              k_scale, v_scale)


def qk_norm_rope_and_cache(qkv: torch.Tensor, q_gamma: torch.Tensor, k_gamma: torch.Tensor, eps: float,
                           positions: torch.Tensor, cos_sin: Optional[torch.Tensor], k_cache: torch.Tensor,
                           v_cache: torch.Tensor, slot_mapping: torch.Tensor, n_heads: int, n_kv_heads: int,
                           head_dim: int, k_scale: float = 1.0, v_scale: float = 1.0) -> torch.Tensor:
    """:func:`rope_and_cache` with Qwen3's per-head RMSNorm of q and k (``q_gamma`` / ``k_gamma``
    ``[head_dim]``, ``eps``) before the rotation: csrc/qk_norm_rope.hip, one wave per (token, head);
    ``head_dim`` 64 or 128. ``qkv`` may be a column slice of wider rows; it is only read."""
    if _use_native(qkv):
        q = torch.empty(qkv.shape[0], n_heads, head_dim, dtype=qkv.dtype, device=qkv.device)
        cs = cos_sin if cos_sin is not None else torch.empty(0, device=qkv.device)
        if ref.is_fp8_cache(k_cache, v_cache):
            native().qk_norm_rope_and_cache_fp8(q, qkv, q_gamma, k_gamma, float(eps), positions, cs, k_cache, v_cache,
                                                slot_mapping, n_heads, n_kv_heads, head_dim, float(k_scale),
                                                float(v_scale))
        else:
            native().qk_norm_rope_and_cache(q, qkv, q_gamma, k_gamma, float(eps), positions, cs, k_cache, v_cache,
                                            slot_mapping, n_heads, n_kv_heads, head_dim)
        return q
    return ref.qk_norm_rope_and_cache(qkv, q_gamma, k_gamma, eps, positions, cos_sin, k_cache, v_cache, slot_mapping,
                                      n_heads, n_kv_heads, head_dim, k_scale, v_scale)


# Limits of the decode attention kernels, repeated from csrc/attn_core.h (GROUP_COLS, MAXS, PLAN_HDR)
# because the CPU path imports without the native module, which exports them as ATTN_GROUP_COLS,
# ATTN_MAX_SPLITS and ATTN_PLAN_HDR (tests/test_kernels_gpu.py holds the two together).
MAX_GROUP_COLS = 16      # MFMA columns a shared-prefix group's query heads may fill (n * G)
MAX_SPLITS = 64          # key splits per (sequence, kv head)
PLAN_HDR = 8             # header ints of an attention plan row


# attention plan row: the header ints + 512 block ids (the 8 waves x 64 lanes of an item's first
# block-id fetch; an item with more tiles reads the rest from the block tables)
PLAN_STRIDE = PLAN_HDR + 512


def plan_enabled() -> bool:
    """Per-step attention plan (``ROUNDTABLE_ATTN_PLAN=0`` turns it off: A/B)."""
    return os.environ.get("ROUNDTABLE_ATTN_PLAN", "1") != "0"


class DecodeWorkspace:
    """Split-KV scratch for paged decode (static: allocated once, reused inside hipGraphs).

    ``max_group``: largest shared-prefix group (knights reading the same KV prefix, see
    :func:`decode_groups`); each (sequence, head) then receives up to ``max_group * max_splits``
    partials, so the partial buffers are strided by ``slot_stride`` = that product."""

    def __init__(self, max_batch: int, n_heads: int, head_dim: int, max_splits: int, device, max_group: int = 1):
        self.max_splits = max_splits
        self.max_group = max(1, max_group)
        self.slot_stride = max_splits * self.max_group
        self.partial_o = torch.empty(max_batch * n_heads * self.slot_stride * head_dim, dtype=torch.float32,
                                     device=device)
        self.partial_ml = torch.empty(max_batch * n_heads * self.slot_stride * 4, dtype=torch.float32, device=device)
        # per-(sequence, kv head) split arrival counters; the kernel re-arms them to 0 itself.
        # Sized by n_heads (>= n_kv_heads) so one workspace serves every GQA ratio.
        self.counters = torch.zeros(max_batch * n_heads, dtype=torch.int32, device=device)
        # persistent / experiment kernels: phase counters (self-re-arming) and the poll-expiry flag
        # (tools/experiments: decode_layer.hip, combine_o.hip)
        self.sync = torch.zeros(8, dtype=torch.int32, device=device)
        self.err = torch.zeros(1, dtype=torch.int32, device=device)
        # per-step attention work plan (attn_plan): per item (sequence, split) a header + the
        # item's block ids; written once per decode step, read by every layer's launch
        self.plan_stride = PLAN_STRIDE
        self.plan = torch.empty(max_batch * max_splits * PLAN_STRIDE, dtype=torch.int32, device=device)
        self.planned = False


_CUS: dict = {}


def device_cus(device=None) -> int:
    """Compute units of ``device`` (the current GPU; 256 = MI355X when no GPU is visible)."""
    if not torch.cuda.is_available():
        return 256
    idx = torch.cuda.current_device() if device is None else torch.device(device).index or 0
    if idx not in _CUS:
        _CUS[idx] = int(torch.cuda.get_device_properties(idx).multi_processor_count)
    return _CUS[idx]


def decode_splits(batch: int, n_kv_heads: int, num_cus: Optional[int] = None, max_splits: int = MAX_SPLITS,
                  grouped: bool = False) -> int:
    """Split-KV count fixed per (batch bucket, kv heads): at most one 8-wave workgroup per CU
    (measured on MI355X, profiles/r01_microbench_v1.log: B=3, ctx 6000 -> 8 splits 22 µs,
    11 splits 27 µs, 16 splits 28 µs; extra workgroups only add hand-off round trips).

    The kernel derives each split's key range from the *runtime* context length, so one
    captured hipGraph serves every length (splits past the end are empty and skipped by the
    combine) — no re-capture as a knight's discussion grows."""
    # grouped (shared-prefix) decode takes the whole chip too. Round 2 measured 3/4 of the CUs best
    # for the 3-knight table (B=3, shared 22K/40K: 8 splits 30.8/42.7 us vs 10 splits 31.7/43.8,
    # r2_gattn_v1.log); with the round-5 copy-free K/V loop the whole chip wins (8 -> 10 splits:
    # 29.0 -> 28.2 / 42.4 -> 40.9 us; driver-config bench 837.1 -> 840.1 tok/s, mean of three
    # same-box passes), and for larger tables by far (16 knights: 1 -> 2 splits 47.5 -> 29.9 us;
    # profiles/r05/attn_splits_large_tables.md).
    # A lone sequence (B = 1: sequential rounds) shares nothing, so it takes the whole chip: B = 1,
    # Llama-3-8B, 10K / 25K / 40K keys: 24 splits 15.9 / 26.3 / 36.8 us, 32 splits 15.0 / 25.9 /
    # 35.7 (profiles/r03/attn_b1_splits.md)
    num_cus = device_cus() if num_cus is None else num_cus
    # ROUNDTABLE_GROUPED_CU_FRACTION: A/B knob for the grouped share of the CUs (default: all)
    frac = float(os.environ.get("ROUNDTABLE_GROUPED_CU_FRACTION", "1.0"))
    cus = int(num_cus * frac) if grouped and batch > 1 else num_cus
    want = cus // max(1, batch * n_kv_heads)        # never more workgroups than CUs: a second
    return int(max(1, min(max_splits, want)))       # wave of workgroups doubles the tail


def decode_groups(group_of: list, shared_blocks: list, G: int) -> Tuple[torch.Tensor, int]:
    """Per-sequence ``[B, 3]`` int32 ``{first sequence, group size n, shared full blocks}`` for
    the shared-prefix decode kernel, from a group label per sequence (members must be
    consecutive; ``None`` = alone) and each group's shared block count. Groups wider than the
    MFMA columns (n * G > 16) are cut into consecutive sub-groups of the same prefix. Returns
    the table and the largest n."""
    B = len(group_of)
    out = torch.zeros(B, 3, dtype=torch.int32)
    cap = max(1, MAX_GROUP_COLS // max(1, G))
    b, nmax = 0, 1
    while b < B:
        e = b + 1
        if group_of[b] is not None:
            while e < B and group_of[e] == group_of[b] and e - b < cap:
                e += 1
        n = e - b
        sh = int(shared_blocks[b]) if n > 1 else 0
        if sh <= 0:
            n, e, sh = 1, b + 1, 0
        for i in range(b, e):
            out[i] = torch.tensor([b, n, sh], dtype=torch.int32)
        nmax = max(nmax, n)
        b = e
    return out, nmax


def paged_attention_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                           block_tables: torch.Tensor, ctx_lens: torch.Tensor, scale: float,
                           num_splits: int = 1, workspace: Optional[DecodeWorkspace] = None,
                           out: Optional[torch.Tensor] = None, groups: Optional[torch.Tensor] = None,
                           planned: bool = False, k_scale: float = 1.0, v_scale: float = 1.0) -> torch.Tensor:
    """``groups`` (optional, device ``[B, 3]`` int32 from :func:`decode_groups`): sequences whose
    block tables share leading blocks decode those keys once for the whole group. The result is
    identical to decoding every sequence alone (the fp32 oracle ignores ``groups``).
    ``planned``: the workspace holds this step's :func:`attn_plan` for exactly these arguments.
    ``k_scale`` / ``v_scale``: read only with an fp8 cache (uint8, kv_dtype "fp8"; head_dim 128)."""
    if _use_native(q):
        if out is None:
            out = torch.empty_like(q)
        G = q.shape[1] // k_cache.shape[1]
        if workspace is None:
            workspace = DecodeWorkspace(q.shape[0], q.shape[1], q.shape[2], max(1, num_splits), q.device,
                                        max_group=MAX_GROUP_COLS // G if groups is not None else 1)
        if groups is not None and (workspace.max_group < MAX_GROUP_COLS // G or workspace.max_splits < num_splits):
            raise ValueError(f"decode workspace too small for shared-prefix groups (max_group "
                             f"{workspace.max_group} < {MAX_GROUP_COLS // G})")
        plan = workspace.plan if planned else None
        if ref.is_fp8_cache(k_cache, v_cache):
            native().paged_attention_decode_fp8(out, q, k_cache, v_cache, block_tables, ctx_lens, scale,
                                                int(num_splits), workspace.partial_o, workspace.partial_ml,
                                                workspace.counters, groups,
                                                workspace.slot_stride if groups is not None else 0,
                                                plan, workspace.plan_stride if planned else 0,
                                                float(k_scale), float(v_scale))
            return out
        native().paged_attention_decode(out, q, k_cache, v_cache, block_tables, ctx_lens, scale,
                                        int(num_splits), workspace.partial_o, workspace.partial_ml,
                                        workspace.counters, groups,
                                        workspace.slot_stride if groups is not None else 0, False,
                                        plan, workspace.plan_stride if planned else 0)
        return out
    return ref.paged_attention_decode(q, k_cache, v_cache, block_tables, ctx_lens, scale, k_scale, v_scale)


def attn_plan(block_tables: torch.Tensor, ctx_lens: torch.Tensor, num_splits: int, workspace: DecodeWorkspace,
              n_heads: int, n_kv_heads: int, groups: Optional[torch.Tensor] = None, batch: Optional[int] = None) -> bool:
    """Write the per-step decode-attention work plan into ``workspace`` (csrc/attention_decode.hip
    attn_plan_kernel): every layer's :func:`paged_attention_decode` of this step (same block tables,
    lengths, groups, splits) then passes ``planned=True`` and starts its K/V stream one dependent
    round trip earlier. Returns whether a plan was written (GPU + native + enabled)."""
    if workspace is None or not block_tables.is_cuda or not native_available() or not plan_enabled():
        return False
    B = int(batch if batch is not None else ctx_lens.numel())
    if B * num_splits * workspace.plan_stride > workspace.plan.numel():
        return False
    native().attn_plan(workspace.plan, workspace.plan_stride, block_tables, ctx_lens, groups, B, int(n_heads),
                       int(n_kv_heads), int(num_splits))
    return True


def prefill_tile_map(cu_q: torch.Tensor, rows_per_tile: int, start_pos=None) -> torch.Tensor:
    """[n_tiles, 2] int32 (sequence, first row) work list for the varlen prefill kernel,
    heaviest tiles first: under the causal mask a tile's work grows with its last key, and
    workgroups start in list order, so the long tiles begin at once and the short ones fill
    the tail (T=4096: 1.3x less time than row order)."""
    items = []
    cq = cu_q.tolist()
    sp = start_pos.tolist() if start_pos is not None else [0] * (len(cq) - 1)
    for s in range(len(cq) - 1):
        for r in range(cq[s], cq[s + 1], rows_per_tile):
            last_key = sp[s] + min(r + rows_per_tile, cq[s + 1]) - cq[s]
            items.append((last_key, s, r))
    items.sort(key=lambda x: -x[0])
    return torch.tensor([(s, r) for _, s, r in items], dtype=torch.int32).reshape(-1, 2)


PREFILL_KT = 64          # keys per tile of the 32x32 prefill kernel (attention_prefill32.hip)


def prefill_split_plan(cu_q: torch.Tensor, rows_per_tile: int, start_pos, n_kv_heads: int,
                       num_cus: Optional[int] = None, min_chunk_tiles: int = 8):
    """Key-split work list for the varlen prefill kernel when its whole tiles would leave CUs idle
    (tensor-parallel shards: one or two KV heads per rank give ``tiles x Hkv`` << CUs, e.g. 28
    workgroups for a 1.8K-token prefill at tp 8). Returns None when the tiles alone fill half the
    chip; else ``(items [n, 5], cmap [m, 4], parts)``: items = (sequence, first row, first / end
    key tile of 64 keys, partial slot or -1), heaviest first; a tile longer than the chunk is cut
    into equal key ranges whose partial slots are consecutive and merged by the combine launch
    (cmap = sequence, first row, first slot, parts). Chunk = the tiles' total key work spread over
    ~2 workgroups per CU, at least ``min_chunk_tiles`` key tiles (partials cost a write + read
    of 128 floats per query row and head each)."""
    cq = cu_q.tolist()
    sp = start_pos.tolist() if start_pos is not None else [0] * (len(cq) - 1)
    tiles = []
    for s in range(len(cq) - 1):
        for r in range(cq[s], cq[s + 1], rows_per_tile):
            last_key = sp[s] + min(r + rows_per_tile, cq[s + 1]) - cq[s]
            tiles.append((s, r, (last_key + PREFILL_KT - 1) // PREFILL_KT))
    num_cus = device_cus() if num_cus is None else num_cus
    hkv = max(1, n_kv_heads)
    if not tiles or len(tiles) * hkv >= num_cus // 2:
        return None
    target = max(1, (2 * num_cus) // hkv)
    total = sum(t[2] for t in tiles)
    chunk = max(min_chunk_tiles, -(-total // target))
    items, cmap, p = [], [], 0
    for s, r, nkt in tiles:
        if nkt <= chunk:
            items.append((nkt, (s, r, 0, nkt, -1)))
            continue
        n = -(-nkt // chunk)
        per = -(-nkt // n)
        cmap.append((s, r, p, n))
        for j in range(n):
            tb = j * per
            te = min(nkt, tb + per)
            items.append((te - tb, (s, r, tb, te, p + j)))
        p += n
    if not cmap:
        return None
    items.sort(key=lambda x: -x[0])
    return (torch.tensor([it for _, it in items], dtype=torch.int32).reshape(-1, 5),
            torch.tensor(cmap, dtype=torch.int32).reshape(-1, 4), p)


def prefill_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_tables: torch.Tensor,
                      cu_q: torch.Tensor, start_pos: torch.Tensor, scale: float,
                      tile_map: Optional[torch.Tensor] = None, split=None, k_scale: float = 1.0,
                      v_scale: float = 1.0) -> torch.Tensor:
    """``split``: a device-resident :func:`prefill_split_plan` ``(items, cmap, parts)`` — the
    key-split launch + its combine; ``tile_map`` otherwise (whole tiles).
    ``k_scale`` / ``v_scale``: read only with an fp8 cache (uint8, kv_dtype "fp8"), which has the
    32x32 kernel only: head_dim 128 and a GQA group <= 8, anything else is refused."""
    if _use_native(q):
        nat = native()
        out = torch.empty_like(q)
        if ref.is_fp8_cache(k_cache, v_cache):
            hkv, D = k_cache.shape[1], q.shape[2]
            if split is not None:
                items, cmap, parts = split
                part_o = torch.empty(parts * hkv * 8 * 32 * D, dtype=torch.float32, device=q.device)
                part_ml = torch.empty(parts * hkv * 8 * 32 * 2, dtype=torch.float32, device=q.device)
                nat.prefill_attention_fp8(out, q, k_cache, v_cache, block_tables, cu_q, start_pos, items, scale,
                                          float(k_scale), float(v_scale), cmap, part_o, part_ml, int(parts))
                return out
            if tile_map is None:
                rows = nat.prefill_rows_per_tile(q.shape[1] // hkv, D)
                tile_map = prefill_tile_map(cu_q.cpu(), rows, start_pos.cpu()).to(q.device)
            nat.prefill_attention_fp8(out, q, k_cache, v_cache, block_tables, cu_q, start_pos, tile_map, scale,
                                      float(k_scale), float(v_scale))
            return out
        if split is not None:
            items, cmap, parts = split
            hkv, D = k_cache.shape[1], q.shape[2]
            part_o = torch.empty(parts * hkv * 8 * 32 * D, dtype=torch.float32, device=q.device)
            part_ml = torch.empty(parts * hkv * 8 * 32 * 2, dtype=torch.float32, device=q.device)
            nat.prefill_attention_split(out, q, k_cache, v_cache, block_tables, cu_q, start_pos, items, cmap,
                                        part_o, part_ml, parts, scale)
            return out
        rows = nat.prefill_rows_per_tile(q.shape[1] // k_cache.shape[1], q.shape[2])
        if tile_map is None:
            tile_map = prefill_tile_map(cu_q.cpu(), rows, start_pos.cpu()).to(q.device)
        nat.prefill_attention(out, q, k_cache, v_cache, block_tables, cu_q, start_pos, tile_map, scale)
        return out
    return ref.prefill_attention(q, k_cache, v_cache, block_tables, cu_q.cpu(), start_pos.cpu(), scale, k_scale,
                                 v_scale)


PRO_PLAIN, PRO_NORM, PRO_NORM_ADD = 0, 1, 2
EPI_STORE, EPI_RESID, EPI_SWIGLU, EPI_ROPE = 0, 1, 2, 3


def shuffle_weight(W: torch.Tensor, gamma: Optional[torch.Tensor] = None, rope_heads: int = 0,
                   head_dim: int = 0, swiglu: bool = False) -> torch.Tensor:
    """Decode-weight copy in the MFMA fragment order of csrc/gemm_skinny.hip, with an RMSNorm
    weight ``gamma`` (over K) optionally folded in and, for a qkv weight used with
    :func:`skinny_gemm_rope`, the first ``rope_heads`` heads' rows pair-interleaved. ``swiglu``:
    W = [gate; up] for the SWIGLU epilogue, stored k-step-paired (one contiguous stream per wave).
    On CPU: the row-major ``W * gamma`` (rows permuted the same way; ``swiglu`` changes nothing)."""
    if _use_native(W):
        Ws = torch.empty_like(W)
        native().shuffle_weight(Ws, W.contiguous(), gamma, int(rope_heads), int(head_dim), bool(swiglu))
        return Ws
    return ref.fold_gamma(W, gamma, rope_heads, head_dim)


def kv_block_copy(k: torch.Tensor, v: torch.Tensor, src, dst) -> None:
    """K8: copy whole KV blocks ``src[i] -> dst[i]`` in every layer of both caches (``[L, NB, E]``)
    in one launch (csrc/kv_copy.hip); CPU: indexed copies."""
    if not src:
        return
    if _use_native(k):
        s_t = torch.tensor(list(src), dtype=torch.int32, device=k.device)
        d_t = torch.tensor(list(dst), dtype=torch.int32, device=k.device)
        native().kv_block_copy(k, v, s_t, d_t)
        return
    si, di = torch.tensor(list(src)), torch.tensor(list(dst))
    k[:, di] = k[:, si]
    v[:, di] = v[:, si]


def unshuffle_weight(Ws: torch.Tensor, rope_heads: int = 0, head_dim: int = 0, swiglu: bool = False,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row-major weight back from a :func:`shuffle_weight` copy: the exact inverse permutation
    (a folded RMSNorm gamma stays folded). Lets a knight keep ONLY the shuffled weights resident
    and rebuild each prefill GEMM's row-major operand in a reused scratch buffer."""
    if out is None:
        out = torch.empty_like(Ws)
    if _use_native(Ws):
        native().unshuffle_weight(out, Ws, int(rope_heads), int(head_dim), bool(swiglu))
        return out
    if rope_heads:
        inv = torch.empty(Ws.shape[0], dtype=torch.long)
        inv[ref.rope_row_perm(Ws.shape[0], rope_heads, head_dim)] = torch.arange(Ws.shape[0])
        out.copy_(Ws[inv])
    else:
        out.copy_(Ws)
    return out


# split-K / CU-balanced skinny GEMM workspace: 256 tile counters + 528 floats per tile part, up
# to 1024 parts (split-K: T x S; balanced: 2 x (tile count mod CU count));
# csrc/skinny_plan.h splitk_parts / split_words
SPLIT_WS_INTS = 256 + 1024 * (16 * 16 * 2 + 16)
SPLIT_K, SPLIT_BALANCE = 2, 1     # split_mode bits


def split_workspace(device) -> torch.Tensor:
    """Zeroed workspace for :func:`skinny_gemm` ``split_ws``. Launches on ONE stream may share it
    (its counters return to zero at the end of every call); concurrent launches must not."""
    return torch.zeros(SPLIT_WS_INTS, dtype=torch.int32, device=device)


FP8_K_RECORD = 64        # k elements per fp8 weight record (csrc/skinny_core.h): K must be a multiple
FP8_MAX_ROWS = 32        # fused rows on fp8 weights: two launches of <= 16


def shuffle_weight_fp8(W: torch.Tensor, gamma: Optional[torch.Tensor] = None, rope_heads: int = 0,
                       head_dim: int = 0, swiglu: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """FP8 (OCP e4m3fn) weight-only quantisation of a decode linear: ``(Wq uint8 [N, K], scale
    fp32 [N])`` with one scale per weight row, taken after the RMSNorm ``gamma`` fold
    (:func:`reference.quantize_fp8` is the contract). On the GPU the codes are in the MFMA fragment
    order of csrc/gemm_skinny_fp8.hip; on CPU they stay row-major. Rows (and their scales) are in the
    order the epilogues index them: ``rope_heads`` leading heads pair-interleaved as
    :func:`shuffle_weight`; ``swiglu`` keeps [gate; up]."""
    N, K = W.shape
    if K % FP8_K_RECORD or N % 16:
        raise ValueError(f"fp8 weights need K % {FP8_K_RECORD} == 0 and N % 16 == 0 (got [{N}, {K}])")
    if _use_native(W):
        Wq = torch.empty(N, K, dtype=torch.uint8, device=W.device)
        scale = torch.empty(N, dtype=torch.float32, device=W.device)
        native().shuffle_weight_fp8(Wq, scale, W.contiguous(), gamma, int(rope_heads), int(head_dim), bool(swiglu))
        return Wq, scale
    return ref.quantize_fp8(W, gamma, rope_heads, head_dim)


def unshuffle_weight_fp8(Wq: torch.Tensor, scale: torch.Tensor, rope_heads: int = 0, head_dim: int = 0,
                         swiglu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row-major ``bf16(code * scale)`` in natural row order from a :func:`shuffle_weight_fp8`
    pair: the operand of the prefill / unfused GEMMs (the fp8 twin of :func:`unshuffle_weight`)."""
    if out is None:
        out = torch.empty(Wq.shape, dtype=torch.bfloat16, device=Wq.device)
    if _use_native(Wq):
        native().unshuffle_weight_fp8(out, Wq, scale, int(rope_heads), int(head_dim), bool(swiglu))
        return out
    Wd = ref.dequantize_fp8(Wq, scale)
    if rope_heads:
        inv = torch.empty(Wq.shape[0], dtype=torch.long)
        inv[ref.rope_row_perm(Wq.shape[0], rope_heads, head_dim)] = torch.arange(Wq.shape[0])
        Wd = Wd[inv]
    out.copy_(Wd)
    return out


def _fp8_check(x, Ws, wscale, pro, x2, xout, split_ws, who):
    """The fp8 launch has the one-tile forms only: refuse everything else loudly."""
    if Ws.dtype != torch.uint8:
        raise ValueError(f"{who}: wscale given but Ws is {Ws.dtype}, not the uint8 codes of shuffle_weight_fp8")
    if pro not in (PRO_PLAIN, PRO_NORM) or x2 is not None or xout is not None:
        raise ValueError(f"{who}: fp8 weights take the PLAIN / NORM prologues only (no x2 / xout)")
    if split_ws is not None:
        raise ValueError(f"{who}: fp8 weights have no split-K / CU-balanced launch (pass split_ws=None)")
    if x.shape[0] > FP8_MAX_ROWS:
        raise ValueError(f"{who}: at most {FP8_MAX_ROWS} rows on fp8 weights (got {x.shape[0]})")
    if x.shape[1] % FP8_K_RECORD:
        raise ValueError(f"{who}: fp8 weights need K % {FP8_K_RECORD} == 0 (got {x.shape[1]})")


MXFP4_K_RECORD = 128     # k elements per mxfp4 weight record (csrc/skinny_core.h): K must be a multiple
MXFP4_MAX_ROWS = 32      # fused rows on mxfp4 weights: two launches of <= 16


def shuffle_weight_mxfp4(W: torch.Tensor, gamma: Optional[torch.Tensor] = None, rope_heads: int = 0,
                         head_dim: int = 0, swiglu: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """MXFP4 (OCP e2m1 codes + one e8m0 scale byte per 32 consecutive k) weight-only quantisation of
    a decode linear: ``(Wq uint8 [N, K/2], scale uint8 [N, K/32])``, taken after the RMSNorm
    ``gamma`` fold (:func:`reference.quantize_mxfp4` is the contract; 17/32 byte per weight). On the
    GPU the codes are in the MFMA fragment order of csrc/gemm_skinny_fp4.hip and the scale bytes in
    the order of its lane records; on CPU both stay row-major. Rows as :func:`shuffle_weight_fp8`."""
    N, K = W.shape
    if K % MXFP4_K_RECORD or N % 16:
        raise ValueError(f"mxfp4 weights need K % {MXFP4_K_RECORD} == 0 and N % 16 == 0 (got [{N}, {K}])")
    if _use_native(W):
        Wq = torch.empty(N, K // 2, dtype=torch.uint8, device=W.device)
        scale = torch.empty(N, K // 32, dtype=torch.uint8, device=W.device)
        native().shuffle_weight_mxfp4(Wq, scale, W.contiguous(), gamma, int(rope_heads), int(head_dim), bool(swiglu))
        return Wq, scale
    return ref.quantize_mxfp4(W, gamma, rope_heads, head_dim)


def unshuffle_weight_mxfp4(Wq: torch.Tensor, scale: torch.Tensor, rope_heads: int = 0, head_dim: int = 0,
                           swiglu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row-major ``bf16(value(code) * 2^(e-127))`` ``[N, K]`` in natural row order from a
    :func:`shuffle_weight_mxfp4` pair: the operand of the prefill / unfused GEMMs."""
    if out is None:
        out = torch.empty(Wq.shape[0], 2 * Wq.shape[1], dtype=torch.bfloat16, device=Wq.device)
    if _use_native(Wq):
        native().unshuffle_weight_mxfp4(out, Wq, scale, int(rope_heads), int(head_dim), bool(swiglu))
        return out
    Wd = ref.dequantize_mxfp4(Wq, scale)
    if rope_heads:
        inv = torch.empty(Wq.shape[0], dtype=torch.long)
        inv[ref.rope_row_perm(Wq.shape[0], rope_heads, head_dim)] = torch.arange(Wq.shape[0])
        Wd = Wd[inv]
    out.copy_(Wd)
    return out


def _mxfp4_check(x, Ws, wscale, pro, x2, xout, split_ws, who):
    """The mxfp4 launch has the one-tile forms only, as fp8: refuse everything else loudly."""
    if Ws.dtype != torch.uint8:
        raise ValueError(f"{who}: uint8 wscale given but Ws is {Ws.dtype}, not the uint8 codes of shuffle_weight_mxfp4")
    if pro not in (PRO_PLAIN, PRO_NORM) or x2 is not None or xout is not None:
        raise ValueError(f"{who}: mxfp4 weights take the PLAIN / NORM prologues only (no x2 / xout)")
    if split_ws is not None:
        raise ValueError(f"{who}: mxfp4 weights have no split-K / CU-balanced launch (pass split_ws=None)")
    if x.shape[0] > MXFP4_MAX_ROWS:
        raise ValueError(f"{who}: at most {MXFP4_MAX_ROWS} rows on mxfp4 weights (got {x.shape[0]})")
    if x.shape[1] % MXFP4_K_RECORD:
        raise ValueError(f"{who}: mxfp4 weights need K % {MXFP4_K_RECORD} == 0 (got {x.shape[1]})")
    if Ws.dim() != 2 or 2 * Ws.shape[1] != x.shape[1] or wscale.numel() * 16 != Ws.numel():
        raise ValueError(f"{who}: mxfp4 weights are codes [N, K/2] with scale bytes [N, K/32] "
                         f"(got {tuple(Ws.shape)} and {tuple(wscale.shape)} for K = {x.shape[1]})")


def skinny_gemm(x: torch.Tensor, Ws: torch.Tensor, pro: int = PRO_PLAIN, epi: int = EPI_STORE,
                res: Optional[torch.Tensor] = None, eps: float = 1e-5, x2: Optional[torch.Tensor] = None,
                xout: Optional[torch.Tensor] = None, split_ws: Optional[torch.Tensor] = None,
                split_mode: int = SPLIT_K | SPLIT_BALANCE,
                wscale: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Decode linear (M <= 16; up to 32 with the plain / norm prologues) on shuffled weights with fused RMSNorm prologue (gamma pre-folded)
    and residual / SwiGLU epilogue. Returns the output (None for RESID, which updates ``res``).
    ``PRO_NORM_ADD``: normalizes ``bf16(x + x2)`` and writes that sum to ``xout`` (TP decode).
    ``split_ws`` (:func:`split_workspace`) enables, per ``split_mode`` bit: ``SPLIT_K`` — fewer
    tiles than CUs (tensor-parallel shards): each tile's K range runs as S workgroups whose last
    arriver combines; ``SPLIT_BALANCE`` — tile count not a multiple of the CU count: the remainder
    tiles run as two K-halves so every CU streams the same bytes.
    ``wscale``: ``Ws`` is the uint8 codes of :func:`shuffle_weight_fp8` and ``wscale`` its scales
    (PLAIN / NORM prologues, no split workspace; 17..32 rows run as two launches of <= 16, rows
    being independent in every epilogue). A uint8 ``wscale``: ``Ws`` / ``wscale`` are the codes and
    block scale bytes of :func:`shuffle_weight_mxfp4`, with the same restrictions."""
    if wscale is not None and wscale.dtype == torch.uint8:
        _mxfp4_check(x, Ws, wscale, pro, x2, xout, split_ws, "skinny_gemm")
        if not _use_native(x):
            return ref.skinny_gemm(x, ref.dequantize_mxfp4(Ws, wscale), pro, epi, res, eps)
        M = x.shape[0]
        n = Ws.shape[0] // (2 if epi == EPI_SWIGLU else 1)
        out = torch.empty(M, n, dtype=x.dtype, device=x.device) if epi != EPI_RESID else x
        for a in range(0, M, 16):
            b = min(M, a + 16)
            native().skinny_gemm_mxfp4(out[a:b], x[a:b], Ws, wscale, pro, epi, res[a:b] if res is not None else None,
                                       eps)
        return None if epi == EPI_RESID else out
    if wscale is not None:
        _fp8_check(x, Ws, wscale, pro, x2, xout, split_ws, "skinny_gemm")
        if not _use_native(x):
            return ref.skinny_gemm(x, ref.dequantize_fp8(Ws, wscale), pro, epi, res, eps)
        M = x.shape[0]
        n = Ws.shape[0] // (2 if epi == EPI_SWIGLU else 1)
        out = torch.empty(M, n, dtype=x.dtype, device=x.device) if epi != EPI_RESID else x
        for a in range(0, M, 16):
            b = min(M, a + 16)
            native().skinny_gemm_fp8(out[a:b], x[a:b], Ws, wscale, pro, epi, res[a:b] if res is not None else None,
                                     eps)
        return None if epi == EPI_RESID else out
    if Ws.dtype == torch.uint8:
        raise ValueError("skinny_gemm: uint8 (fp8 / mxfp4) weights need their wscale")
    if _use_native(x):
        n = Ws.shape[0] // (2 if epi == EPI_SWIGLU else 1)
        out = torch.empty(x.shape[0], n, dtype=x.dtype, device=x.device) if epi != EPI_RESID else x
        native().skinny_gemm(out, x, Ws, pro, epi, res, eps, x2, xout, split_ws, int(split_mode))
        return None if epi == EPI_RESID else out
    return ref.skinny_gemm(x, Ws, pro, epi, res, eps, x2, xout)


def skinny_gemm_rope(x: torch.Tensor, Ws: torch.Tensor, pro: int, positions: torch.Tensor, cos_sin: torch.Tensor,
                     k_cache: torch.Tensor, v_cache: torch.Tensor, slots: torch.Tensor, n_heads: int,
                     n_kv_heads: int, head_dim: int, eps: float = 1e-5, x2: Optional[torch.Tensor] = None,
                     xout: Optional[torch.Tensor] = None, split_ws: Optional[torch.Tensor] = None,
                     split_mode: int = SPLIT_K | SPLIT_BALANCE, bias: Optional[torch.Tensor] = None,
                     wscale: Optional[torch.Tensor] = None, k_scale: float = 1.0,
                     v_scale: float = 1.0) -> torch.Tensor:
    """Decode qkv projection (+ optional RMSNorm prologue) with RoPE and the paged K/V cache
    write fused into the epilogue; returns q [M, n_heads, head_dim]. ``Ws`` must come from
    ``shuffle_weight(Wqkv, gamma, rope_heads=n_heads + n_kv_heads, head_dim=head_dim)``.
    ``split_ws`` / ``split_mode``: as in :func:`skinny_gemm` (no balanced launch with ``PRO_NORM_ADD``).
    ``bias`` (Qwen2 q/k/v bias, added after the norm scale and before RoPE) must come from
    :func:`rope_bias` (fp32, the shuffled weight's column order).
    ``wscale``: fp8 weights, as in :func:`skinny_gemm` (``Ws`` from ``shuffle_weight_fp8`` with the
    same ``rope_heads`` / ``head_dim``; uint8 ``wscale``: from ``shuffle_weight_mxfp4``).
    ``k_scale`` / ``v_scale``: read only with an fp8 cache (uint8, kv_dtype "fp8"): the epilogue then
    stores ``kv_fp8_code`` of its finished fp32 sums (after bias and RoPE), for every weight type."""
    ks = (float(k_scale), float(v_scale))
    if wscale is not None and wscale.dtype == torch.uint8:
        _mxfp4_check(x, Ws, wscale, pro, x2, xout, split_ws, "skinny_gemm_rope")
        if not _use_native(x):
            return ref.skinny_gemm_rope(x, ref.dequantize_mxfp4(Ws, wscale), pro, positions, cos_sin, k_cache,
                                        v_cache, slots, n_heads, n_kv_heads, head_dim, eps, None, None, bias, *ks)
        M = x.shape[0]
        q = torch.empty(M, n_heads, head_dim, dtype=x.dtype, device=x.device)
        kv8 = ref.is_fp8_cache(k_cache, v_cache)
        for a in range(0, M, 16):
            b = min(M, a + 16)
            if kv8:
                native().skinny_gemm_rope_kv8(q[a:b], x[a:b], Ws, wscale, pro, positions[a:b], cos_sin, k_cache,
                                              v_cache, slots[a:b], n_heads, n_kv_heads, head_dim, eps, bias=bias,
                                              k_scale=ks[0], v_scale=ks[1])
                continue
            native().skinny_gemm_rope_mxfp4(q[a:b], x[a:b], Ws, wscale, pro, positions[a:b], cos_sin, k_cache,
                                            v_cache, slots[a:b], n_heads, n_kv_heads, head_dim, eps, bias)
        return q
    if wscale is not None:
        _fp8_check(x, Ws, wscale, pro, x2, xout, split_ws, "skinny_gemm_rope")
        if not _use_native(x):
            return ref.skinny_gemm_rope(x, ref.dequantize_fp8(Ws, wscale), pro, positions, cos_sin, k_cache,
                                        v_cache, slots, n_heads, n_kv_heads, head_dim, eps, None, None, bias, *ks)
        M = x.shape[0]
        q = torch.empty(M, n_heads, head_dim, dtype=x.dtype, device=x.device)
        kv8 = ref.is_fp8_cache(k_cache, v_cache)
        for a in range(0, M, 16):
            b = min(M, a + 16)
            if kv8:
                native().skinny_gemm_rope_kv8(q[a:b], x[a:b], Ws, wscale, pro, positions[a:b], cos_sin, k_cache,
                                              v_cache, slots[a:b], n_heads, n_kv_heads, head_dim, eps, bias=bias,
                                              k_scale=ks[0], v_scale=ks[1])
                continue
            native().skinny_gemm_rope_fp8(q[a:b], x[a:b], Ws, wscale, pro, positions[a:b], cos_sin, k_cache, v_cache,
                                          slots[a:b], n_heads, n_kv_heads, head_dim, eps, bias)
        return q
    if Ws.dtype == torch.uint8:
        raise ValueError("skinny_gemm_rope: uint8 (fp8 / mxfp4) weights need their wscale")
    if _use_native(x):
        q = torch.empty(x.shape[0], n_heads, head_dim, dtype=x.dtype, device=x.device)
        if ref.is_fp8_cache(k_cache, v_cache):
            native().skinny_gemm_rope_kv8(q, x, Ws, None, pro, positions, cos_sin, k_cache, v_cache, slots, n_heads,
                                          n_kv_heads, head_dim, eps, x2, xout, split_ws, int(split_mode), bias,
                                          ks[0], ks[1])
            return q
        native().skinny_gemm_rope(q, x, Ws, pro, positions, cos_sin, k_cache, v_cache, slots, n_heads, n_kv_heads,
                                  head_dim, eps, x2, xout, split_ws, int(split_mode), bias)
        return q
    return ref.skinny_gemm_rope(x, Ws, pro, positions, cos_sin, k_cache, v_cache, slots, n_heads, n_kv_heads,
                                head_dim, eps, x2, xout, bias, *ks)


def rope_bias(b: torch.Tensor, n_heads: int, n_kv_heads: int, head_dim: int) -> torch.Tensor:
    """A q/k/v bias [(n_heads + 2 n_kv_heads) * head_dim] in the form :func:`skinny_gemm_rope` adds it."""
    return ref.rope_bias(b, n_heads + n_kv_heads, head_dim)


def decode_prep(slots: torch.Tensor, offsets: torch.Tensor, res: torch.Tensor, ids: torch.Tensor,
                positions: torch.Tensor, block_tables: torch.Tensor, embed: torch.Tensor, block_size: int) -> None:
    """Captured-step prologue (csrc/decode_step.hip): K/V slots, sampler offsets, embedding rows."""
    if _use_native(ids):
        native().decode_prep(slots, offsets, res, ids, positions, block_tables, embed, int(block_size))
        return
    ref.decode_prep(slots, offsets, res, ids, positions, block_tables, embed, block_size)


def paging_guard(block_tables: torch.Tensor, ctx_lens: torch.Tensor, positions: Optional[torch.Tensor],
                 slots: Optional[torch.Tensor], err: torch.Tensor, num_blocks: int, block_size: int) -> None:
    """Debug-mode device guard of the paging metadata (err[0] |= ref.PAGING_GUARD_CODES bits).

    Capturable: placed inside the decode hipGraph it validates the slots / lengths the graph
    advances on the device, which host-side asserts never see."""
    if _use_native(ctx_lens):
        native().paging_guard(block_tables, ctx_lens, positions, slots, err, int(num_blocks), int(block_size))
        return
    ref.paging_guard(block_tables, ctx_lens, positions, slots, err, num_blocks, block_size)


def paging_guard_message(code: int) -> str:
    return "; ".join(msg for bit, msg in ref.PAGING_GUARD_CODES.items() if code & bit) or "ok"


def decode_advance(out: torch.Tensor, ids: torch.Tensor, positions: torch.Tensor, ctx_lens: torch.Tensor,
                   step: torch.Tensor, nxt: torch.Tensor, prep=None) -> None:
    """Captured-step epilogue: record the sampled ids and advance positions / lengths / step.

    prep = (slots, offsets, res, block_tables, embed, block_size) also runs the NEXT step's
    decode_prep from the advanced ids / positions in the same launch."""
    if _use_native(ids):
        if prep is None:
            native().decode_advance(out, ids, positions, ctx_lens, step, nxt)
        else:
            slots, offsets, res, bt, embed, bs = prep
            native().decode_advance(out, ids, positions, ctx_lens, step, nxt, slots, offsets, res, bt, embed, int(bs))
        return
    ref.decode_advance(out, ids, positions, ctx_lens, step, nxt, prep)


def silu_and_mul(x: torch.Tensor) -> torch.Tensor:
    if _use_native(x):
        out = torch.empty(*x.shape[:-1], x.shape[-1] // 2, dtype=x.dtype, device=x.device)
        native().silu_and_mul(out, x)
        return out
    return ref.silu_and_mul(x)


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    if _use_native(x):
        out = torch.empty_like(x)
        native().gelu_tanh(out, x)
        return out
    return ref.gelu_tanh(x)


def sample_workspace(batch: int, device) -> torch.Tensor:
    """Zeroed K6 workspace for ``batch`` rows: its arrival tickets re-arm themselves after every
    launch, so one persistent workspace serves every replay of a captured step (no memset)."""
    return torch.zeros(native().sample_workspace_floats(batch), dtype=torch.float32, device=device)


def sample(logits: torch.Tensor, temperature: torch.Tensor, top_p: torch.Tensor, top_k: torch.Tensor,
           seeds: torch.Tensor, offsets: torch.Tensor, out: Optional[torch.Tensor] = None,
           ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-row ``offsets`` (int64, device-resident: the knight's position) keep hipGraph replays
    deterministic. ``ws``: a :func:`sample_workspace` (one is zero-allocated per call otherwise)."""
    if _use_native(logits):
        if out is None:
            out = torch.empty(logits.shape[0], dtype=torch.int64, device=logits.device)
        nat = native()
        if ws is None:
            ws = sample_workspace(logits.shape[0], logits.device)
        nat.sample(out, logits, temperature, top_p, top_k, seeds, offsets, ws)
        return out
    return ref.sample(logits, temperature, top_p, top_k, seeds, offsets)


def sample_advance(logits: torch.Tensor, temperature: torch.Tensor, top_p: torch.Tensor, top_k: torch.Tensor,
                   seeds: torch.Tensor, offsets: torch.Tensor, ws: torch.Tensor, nxt: torch.Tensor,
                   out: torch.Tensor, ids: torch.Tensor, positions: torch.Tensor, ctx_lens: torch.Tensor,
                   step: torch.Tensor, slots: torch.Tensor, res: torch.Tensor, block_tables: torch.Tensor,
                   embed: torch.Tensor, block_size: int) -> torch.Tensor:
    """The captured decode step's K6 sampler fused with :func:`decode_advance` + the next step's
    :func:`decode_prep` (one launch): samples ``nxt`` from ``logits`` with the RNG ``offsets``, then
    records it in ``out[step]``, advances ids / positions / lengths / step and writes the next
    step's K/V slots, ``offsets`` and embedding rows."""
    if _use_native(logits):
        native().sample_advance(nxt, logits, temperature, top_p, top_k, seeds, offsets, ws, out, ids, positions,
                                ctx_lens, step, slots, res, block_tables, embed, int(block_size))
        return nxt
    nxt.copy_(ref.sample(logits, temperature, top_p, top_k, seeds, offsets))
    ref.decode_advance(out, ids, positions, ctx_lens, step, nxt, (slots, offsets, res, block_tables, embed,
                                                                  block_size))
    return nxt


LOGIT_PROC_WINDOW = ref.LOGIT_PROC_WINDOW        # tokens the repetition set / the counted reply reach back
LOGIT_PROC_MAX_BIAS = ref.LOGIT_PROC_MAX_BIAS    # logit_bias entries per row


class LogitProc:
    """Static per-row operands of :func:`apply_logit_processors` for a batch of ``batch`` rows, all
    neutral until :meth:`fill`: ``hist`` [B, cap] int32 with ``hist_len`` / ``reply_from`` (the host
    part of each row's token history and where its reply starts in it), ``rp`` / ``last_n`` /
    ``pp`` / ``fp`` and the bias list ``bias_tok`` / ``bias_val`` [B, 300] with ``bias_n``. A decode
    graph owns one and refills it per turn; the captured kernel reads these addresses."""

    def __init__(self, batch: int, device, hist_cap: int = LOGIT_PROC_WINDOW, bias_cap: int = LOGIT_PROC_MAX_BIAS):
        z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=device)      # noqa: E731
        self.hist, self.hist_len, self.reply_from = z(batch, max(1, hist_cap)), z(batch), z(batch)
        self.rp = torch.ones(batch, dtype=torch.float32, device=device)
        self.last_n = z(batch)
        self.pp, self.fp = z(batch, dt=torch.float32), z(batch, dt=torch.float32)
        self.bias_tok, self.bias_val = z(batch, max(1, bias_cap)), z(batch, max(1, bias_cap), dt=torch.float32)
        self.bias_n = z(batch)
        self.active = False

    def fill(self, rows) -> "LogitProc":
        """``rows``: per batch row ``(tokens, reply_start, params)`` — the row's whole host-side
        history, the index in it where the reply starts, and an object with the SamplingParams
        penalty fields — or None for a neutral (padding) row. Keeps the tail that fits ``hist``."""
        B, cap = self.hist.shape
        bcap = self.bias_tok.shape[1]
        hist = torch.zeros(B, cap, dtype=torch.int32)
        ints = torch.zeros(4, B, dtype=torch.int32)            # hist_len, reply_from, last_n, bias_n
        flts = torch.zeros(3, B, dtype=torch.float32)          # rp, pp, fp
        flts[0] = 1.0
        btok = torch.zeros(B, bcap, dtype=torch.int32)
        bval = torch.zeros(B, bcap, dtype=torch.float32)
        self.active = False
        for b, row in enumerate(rows):
            if row is None or not row[2].has_processors():
                continue
            tokens, reply_start, p = row
            self.active = True
            keep = list(tokens[-cap:])
            cut = len(tokens) - len(keep)
            hist[b, :len(keep)] = torch.tensor(keep, dtype=torch.int32)
            bias = list((p.logit_bias or {}).items())
            if len(bias) > bcap:
                raise ValueError(f"logit_bias has {len(bias)} entries; at most {bcap} are supported")
            ints[:, b] = torch.tensor([len(keep), min(max(reply_start - cut, 0), len(keep)), p.repeat_last_n,
                                       len(bias)], dtype=torch.int32)
            flts[:, b] = torch.tensor([p.repetition_penalty, p.presence_penalty, p.frequency_penalty])
            if bias:
                btok[b, :len(bias)] = torch.tensor([int(t) for t, _ in bias], dtype=torch.int32)
                bval[b, :len(bias)] = torch.tensor([float(v) for _, v in bias], dtype=torch.float32)
        dev = self.hist.device
        for dst, src in ((self.hist, hist), (self.hist_len, ints[0]), (self.reply_from, ints[1]),
                         (self.last_n, ints[2]), (self.bias_n, ints[3]), (self.rp, flts[0]), (self.pp, flts[1]),
                         (self.fp, flts[2]), (self.bias_tok, btok), (self.bias_val, bval)):
            dst.copy_(src.to(dev, non_blocking=True))
        return self


def apply_logit_processors(logits: torch.Tensor, proc: LogitProc, out: Optional[torch.Tensor] = None,
                           step: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In place on ``logits`` [B, V] (bf16 or fp32, row stride >= V): logit_bias, then the repetition
    penalty, then frequency / presence penalties, from each row's history
    ``proc.hist[b, :hist_len[b]] ++ out[0:step, b]`` (csrc/logit_proc.hip; semantics:
    ops/reference.py). ``step=None``: host history only. With the graph's ``out`` [steps, B] and
    device ``step`` the call is capturable and reads the tokens K6 recorded in earlier replays."""
    if _use_native(logits):
        native().logit_proc(logits, proc.hist, proc.hist_len, proc.reply_from, proc.rp, proc.last_n, proc.pp, proc.fp,
                            proc.bias_tok, proc.bias_val, proc.bias_n, out if step is not None else None, step)
        return logits
    return ref.apply_logit_processors(logits, proc, out, step)


MAX_TOP_LOGPROBS = ref.MAX_TOP_LOGPROBS          # alternatives a row can ask for


class LogProbs:
    """Static operands and records of :func:`token_logprobs` for ``batch`` rows and ``steps`` record
    rows: ``n_top`` [B] int32 (-1: the row does not ask, the default), the kernels' workspace, and
    the records ``tok_lp`` [steps, B] fp32, ``top_id`` [steps, B, 20] int32, ``top_lp``
    [steps, B, 20] fp32. A decode graph owns one and refills ``n_top`` per turn; the captured
    kernels read and write these addresses."""

    def __init__(self, batch: int, device, steps: int = 1):
        self.n_top = torch.full((batch,), -1, dtype=torch.int32, device=device)
        self.ws = torch.zeros(batch * ref.LOGPROB_WS_ROW, dtype=torch.float32, device=device)
        self.tok_lp = torch.zeros(max(1, steps), batch, dtype=torch.float32, device=device)
        self.top_id = torch.full((max(1, steps), batch, MAX_TOP_LOGPROBS), -1, dtype=torch.int32, device=device)
        self.top_lp = torch.full((max(1, steps), batch, MAX_TOP_LOGPROBS), float("-inf"), dtype=torch.float32,
                                 device=device)
        self.wanted: list = [-1] * batch

    def fill(self, rows) -> "LogProbs":
        """``rows``: per batch row an object with the SamplingParams field ``logprobs`` (None: off,
        n: the chosen token's logprob plus n alternatives), or None for a row that does not ask."""
        want = [-1] * self.n_top.numel()
        for b, p in enumerate(rows):
            n = None if p is None else getattr(p, "logprobs", None)
            if n is not None:
                if not 0 <= int(n) <= MAX_TOP_LOGPROBS:
                    raise ValueError(f"logprobs must be in 0..{MAX_TOP_LOGPROBS}, got {n}")
                want[b] = int(n)
        self.wanted = want
        self.n_top.copy_(torch.tensor(want, dtype=torch.int32).to(self.n_top.device, non_blocking=True))
        return self

    def records(self, n: int = 1):
        """The first ``n`` record rows on the host: per step, per row, ``(tok_lp, top_ids, top_lps)``
        cut to the row's ``n_top``, or None for a row that did not ask."""
        tok = self.tok_lp[:n].cpu().tolist()
        ids = self.top_id[:n].cpu().tolist()
        lps = self.top_lp[:n].cpu().tolist()
        return [[None if k < 0 else (tok[s][b], ids[s][b][:k], lps[s][b][:k]) for b, k in enumerate(self.wanted)]
                for s in range(len(tok))]


def token_logprobs(logits: torch.Tensor, lp: LogProbs, ids: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, step: Optional[torch.Tensor] = None) -> LogProbs:
    """The chosen token's log-probability and the ``n_top`` most likely tokens of each row of
    ``logits`` [B, V] (bf16 or fp32, row stride >= V; only read) into ``lp``'s records, on the
    logits as the sampler saw them: after the logit processors, before temperature / top-k / top-p
    (csrc/logprobs.hip; semantics: ops/reference.py). ``ids`` [B] int64: the chosen tokens, record
    row 0. With the graph's ``out`` [steps, B] and device ``step`` the call is capturable, sits
    AFTER the step's sample and advance, and writes record row ``step - 1`` for ``out[step - 1]``."""
    if (out is None) != (step is None) or (ids is None) == (step is None):
        raise ValueError("token_logprobs takes either ids or (out, step)")
    if _use_native(logits):
        native().token_logprobs(logits, lp.n_top, lp.ws, lp.tok_lp, lp.top_id, lp.top_lp, ids, out, step)
        return lp
    return ref.token_logprobs(logits, lp, ids, out, step)


GRAMMAR_MAX_TABLE = ref.GRAMMAR_MAX_TABLE        # table entries a row's slot holds
GRAMMAR_MAX_STATES = ref.GRAMMAR_MAX_STATES


def _grammar_host_tensors(g):
    """(cls uint8[256], tab int16[n_states * n_classes], accept uint8[n_states]) of a compiled grammar, cached on it."""
    t = getattr(g, "_host_tensors", None)
    if t is None:
        tab = torch.tensor([e - 65536 if e >= 32768 else e for e in g.trans], dtype=torch.int16)
        t = g._host_tensors = (torch.tensor(list(g.cls), dtype=torch.uint8), tab,
                               torch.tensor(list(g.accept), dtype=torch.uint8))
    return t


class GrammarMask:
    """Static per-row operands of :func:`apply_grammar_mask` for ``batch`` rows over one token table
    (``engine.grammar.TokenTable``), no row with a grammar until :meth:`fill`: ``meta`` [B, 8] int32
    (active, n_states, n_classes, the three pop targets, n_stop), ``cls`` [B, 256] uint8, ``tab``
    [B, 65536] int16 (16-bit entries; a row uses the first n_states * n_classes), ``accept`` [B, 4096]
    uint8, ``stops`` [B, 8] int32 and the two-slot ``state`` [2, B, 4] int32 (q, depth, stack), plus
    the table's ``tok_off`` int32 [V + 1] / ``tok_bytes`` uint8. A decode graph owns one and refills it
    per turn; the captured kernel reads these addresses."""

    def __init__(self, batch: int, device, table):
        z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=device)      # noqa: E731
        self.meta, self.cls = z(batch, ref.GRAMMAR_META), z(batch, 256, dt=torch.uint8)
        self.tab = torch.full((batch, GRAMMAR_MAX_TABLE), -1, dtype=torch.int16, device=device)
        self.accept = z(batch, GRAMMAR_MAX_STATES, dt=torch.uint8)
        self.stops = torch.full((batch, ref.GRAMMAR_MAX_STOPS), -1, dtype=torch.int32, device=device)
        self.state = z(2, batch, 4)
        self.table = table
        self.tok_off, self.tok_bytes = table.tensors(device)
        self.active = False

    @staticmethod
    def _state_row(st) -> list:
        q, depth, stack = st
        return [q, depth, stack - (1 << 32) if stack >= (1 << 31) else stack, 0]

    def fill(self, rows) -> "GrammarMask":
        """``rows``: per batch row ``(bound, state)`` — an ``engine.grammar.BoundGrammar`` over this
        mask's token table and the row's CURRENT state ``(q, depth, stack)`` (the start state advanced
        over the reply tokens the host holds) — or None for a row without a grammar."""
        B = self.meta.shape[0]
        meta = torch.zeros(B, ref.GRAMMAR_META, dtype=torch.int32)
        stops = torch.full((B, ref.GRAMMAR_MAX_STOPS), -1, dtype=torch.int32)
        state = torch.zeros(2, B, 4, dtype=torch.int32)
        cls = torch.zeros(B, 256, dtype=torch.uint8)
        dev = self.meta.device
        self.active = False
        for b, row in enumerate(rows):
            if row is None:
                continue
            bound, st = row
            if bound.table is not self.table:
                raise ValueError("the grammar is bound to another token table")
            g = bound.g
            self.active = True
            c, tab, acc = _grammar_host_tensors(g)
            sids = list(bound.table.stop_ids)
            meta[b] = torch.tensor([1, g.n_states, g.n_classes, *g.pop_target, len(sids), 0], dtype=torch.int32)
            stops[b, :len(sids)] = torch.tensor(sids, dtype=torch.int32)
            state[0, b] = torch.tensor(self._state_row(st), dtype=torch.int32)
            cls[b] = c
            self.tab[b, :tab.numel()].copy_(tab.to(dev, non_blocking=True))
            self.accept[b, :acc.numel()].copy_(acc.to(dev, non_blocking=True))
        for dst, src in ((self.meta, meta), (self.stops, stops), (self.state, state), (self.cls, cls)):
            dst.copy_(src.to(dev, non_blocking=True))
        return self

    def set_states(self, states) -> "GrammarMask":
        """Slot 0 of ``state`` only: per row a state or None (the eager path's per-step update)."""
        rows = torch.tensor([[0, 0, 0, 0] if st is None else self._state_row(st) for st in states], dtype=torch.int32)
        self.state[0, :rows.shape[0]].copy_(rows.to(self.state.device, non_blocking=True))
        return self

    def states(self, slot: int):
        """Slot ``slot`` on the host: per row ``(q, depth, stack)``."""
        return [(q, d, s & 0xFFFFFFFF) for q, d, s, _ in self.state[slot].cpu().tolist()]


def apply_grammar_mask(logits: torch.Tensor, gm: GrammarMask, out: Optional[torch.Tensor] = None,
                       step: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In place on ``logits`` [B, V] (bf16 or fp32, row stride >= V): ``-inf`` over every token the row's
    grammar cannot accept next (csrc/grammar_mask.hip; semantics: ops/reference.py); allowed
    elements, rows without a grammar and columns past V are not written. ``step=None``: each row's
    state is slot 0 of ``gm.state``, as :meth:`GrammarMask.fill` / ``set_states`` left it. With the
    graph's ``out`` [steps, B] and device ``step`` the call is capturable: at ``step = s > 0`` the state
    is slot ``(s - 1) & 1`` advanced over the token K6 recorded at ``out[s - 1, b]``, stored to slot
    ``s & 1``."""
    if logits.shape[1] > gm.table.vocab:
        raise ValueError(f"the token table covers {gm.table.vocab} ids, the logits have {logits.shape[1]}")
    if _use_native(logits):
        native().grammar_mask(logits, gm.meta, gm.cls, gm.tab, gm.accept, gm.stops, gm.state, gm.tok_off,
                              gm.tok_bytes, out if step is not None else None, step)
        return logits
    return ref.apply_grammar_mask(logits, gm, out if step is not None else None, step)


class GrammarBudgetMask(GrammarMask):
    """:class:`GrammarMask` plus what the budgeted launch reads per row: ``budget`` [B] int32 (tokens the
    row may still emit when the launch's step is 0), ``need`` [2, B, 4096] int16 (16-bit ``c_acc`` /
    ``c_pop`` entries of ``engine.grammar.GrammarBudget``), ``all_live`` [B, 4096] uint8 and ``need_cap`` in
    ``meta[:, 7]``. A row given without a budget gets ``BUDGET_FREE`` and zero need arrays: nothing binds
    and its mask is :func:`apply_grammar_mask`'s."""

    def __init__(self, batch: int, device, table):
        super().__init__(batch, device, table)
        self.budget = torch.full((batch,), ref.GRAMMAR_BUDGET_FREE, dtype=torch.int32, device=device)
        self.need = torch.zeros(2, batch, GRAMMAR_MAX_STATES, dtype=torch.int16, device=device)
        self.all_live = torch.zeros(batch, GRAMMAR_MAX_STATES, dtype=torch.uint8, device=device)

    def fill(self, rows) -> "GrammarBudgetMask":
        """``rows``: per batch row ``(bound, state, budget)`` or None; ``budget`` None for a row nothing
        bounds, else ``max_new_tokens`` less the reply tokens the host holds (``state`` is the state
        after them). ValueError from ``bound.budget()`` for a pair that cannot finish inside a budget."""
        super().fill([None if r is None else (r[0], r[1]) for r in rows])
        self._ref_rows = {}      # (ops/reference.py keeps each row's host copy between fills)
        B = self.meta.shape[0]
        dev = self.meta.device
        budget = torch.full((B,), ref.GRAMMAR_BUDGET_FREE, dtype=torch.int32)
        cap = torch.zeros(B, dtype=torch.int32)
        for b, row in enumerate(rows):
            if row is None:
                continue
            bound, _, left = row
            n = bound.g.n_states
            need = torch.zeros(2, n, dtype=torch.int16)
            if left is not None:
                bd = bound.budget()
                budget[b] = max(-1, min(int(left), ref.GRAMMAR_BUDGET_FREE))
                cap[b] = min(bd.need_cap, ref.GRAMMAR_NEED_INF)
                need = _need_host_tensor(bd)
            self.need[:, b, :n].copy_(need.to(dev, non_blocking=True))
            self.all_live[b, :n].copy_(torch.tensor(list(bound.all_live()), dtype=torch.uint8).to(dev, non_blocking=True))
        self.budget.copy_(budget.to(dev, non_blocking=True))
        self.meta[:, 7].copy_(cap.to(dev, non_blocking=True))
        return self

    def set_budgets(self, budgets) -> "GrammarBudgetMask":
        """``budget`` only: per row the tokens left, or None for a row nothing bounds (the eager path's
        per-step update, beside :meth:`set_states`)."""
        v = torch.tensor([ref.GRAMMAR_BUDGET_FREE if x is None else max(-1, min(int(x), ref.GRAMMAR_BUDGET_FREE))
                          for x in budgets], dtype=torch.int32)
        self.budget[:v.shape[0]].copy_(v.to(self.budget.device, non_blocking=True))
        return self


def _need_host_tensor(bd):
    """int16 [2, n_states] (c_acc, c_pop as 16-bit entries) of a GrammarBudget, cached on it."""
    t = getattr(bd, "_host_need", None)
    if t is None:
        t = bd._host_need = torch.tensor([[e - 65536 if e >= 32768 else e for e in arr] for arr in (bd.c_acc, bd.c_pop)],
                                         dtype=torch.int16)
    return t


def apply_grammar_mask_budget(logits: torch.Tensor, gm: GrammarBudgetMask, out: Optional[torch.Tensor] = None,
                              step: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`apply_grammar_mask` under each row's token budget (csrc/grammar_budget.hip; semantics:
    ops/reference.py): with ``r = gm.budget[b] - step`` tokens left, a non-stop token is allowed iff its walk
    stays live and ``need(state after it) <= r - 2``; ``r <= 0`` allows stop ids only. In a state flagged
    all-live with ``need_cap <= r - 2`` the kernel walks no token. Capturable with ``out`` and ``step``."""
    if logits.shape[1] > gm.table.vocab:
        raise ValueError(f"the token table covers {gm.table.vocab} ids, the logits have {logits.shape[1]}")
    if _use_native(logits):
        native().grammar_mask_budget(logits, gm.meta, gm.cls, gm.tab, gm.accept, gm.stops, gm.state, gm.tok_off,
                                     gm.tok_bytes, gm.budget, gm.need, gm.all_live, out if step is not None else None, step)
        return logits
    return ref.apply_grammar_mask_budget(logits, gm, out if step is not None else None, step)
