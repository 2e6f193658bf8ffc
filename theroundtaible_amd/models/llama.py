"""Llama-3 / Mistral / Qwen2 / Qwen3 decoder (dense, GQA, RoPE, SwiGLU, RMSNorm; Qwen2: q/k/v bias;
Qwen3: a per-head RMSNorm of q and k before RoPE, ``cfg.qk_norm``), TP-aware.

Per layer (decode and prefill share the code; only the attention op differs):

    x, res = fused_add_rms_norm(h, res)          K1 (HIP)
    qkv    = x @ Wqkv^T                          hipBLASLt (column-parallel)
    q      = rope_and_cache(qkv, ...)            K2 (HIP): RoPE on q/k + paged K/V scatter
             (Qwen3: qk_norm_rope_and_cache      K2n (HIP): per-head q/k RMSNorm first)
    a      = paged_decode | prefill attention    K3 / K4 (HIP, MFMA)
    h      = a @ Wo^T ; all_reduce               hipBLASLt (row-parallel) + RCCL (C2)
    x, res = fused_add_rms_norm(h, res)          K1
    h      = silu_and_mul(x @ Wgu^T) @ Wd^T      hipBLASLt + K5 (HIP) + hipBLASLt ; all_reduce
    logits = final_norm(h) @ Wlm^T ; all_gather  hipBLASLt (vocab-parallel) + RCCL (C3)
"""
from __future__ import annotations

import os

import math
from dataclasses import dataclass
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from .. import ops
from ..ops.reference import rope_cos_sin
from ..parallel.tp import TPInfo
from .config import ModelConfig


@dataclass
class AttnMeta:
    """Per-forward attention metadata (device tensors)."""
    kind: str                               # "decode" | "prefill"
    slot_mapping: torch.Tensor              # [T] int64
    block_tables: torch.Tensor              # [S, max_blocks] int32
    ctx_lens: Optional[torch.Tensor] = None     # decode: [B] int32
    num_splits: int = 1                         # decode split-KV
    workspace: Optional[ops.DecodeWorkspace] = None
    cu_q: Optional[torch.Tensor] = None         # prefill: [S+1] int32
    start_pos: Optional[torch.Tensor] = None    # prefill: [S] int32
    tile_map: Optional[torch.Tensor] = None     # prefill: [n_tiles, 2] int32
    prefill_split: Optional[tuple] = None       # prefill: ops.prefill_split_plan (items, cmap, parts) on device
    last_rows: Optional[torch.Tensor] = None    # prefill: rows whose logits are needed
    groups: Optional[torch.Tensor] = None       # decode: [B, 3] shared-prefix groups (ops.decode_groups)
    local_logits: bool = False                  # TP decode: return this rank's vocab shard (C3 greedy argmax)
    planned: bool = False                       # decode: the workspace holds this step's ops.attn_plan


class LlamaModel:
    def __init__(self, cfg: ModelConfig, weights: Dict[str, torch.Tensor], device, dtype=torch.bfloat16,
                 tp: Optional[TPInfo] = None):
        self.cfg = cfg
        self.w = weights
        self.tp = tp or TPInfo()
        self.device = device
        self.dtype = dtype
        if cfg.n_heads % self.tp.size or cfg.ffn % self.tp.size:
            raise ValueError(f"{cfg.name}: {cfg.n_heads} heads / FFN {cfg.ffn} do not split over tp={self.tp.size}")
        self.n_heads = cfg.n_heads // self.tp.size
        self.n_kv_heads = self.tp.kv_heads(cfg.n_kv_heads)   # replicated when tp > KV heads
        self.head_dim = cfg.head_dim
        self.scale = 1.0 / math.sqrt(cfg.head_dim)
        self.cos_sin = rope_cos_sin(cfg.max_pos, cfg.head_dim, cfg.rope_theta, device, cfg.rope_scaling)
        self.layers = [{k.split(".", 2)[2]: v for k, v in weights.items() if k.startswith(f"layers.{i}.")}
                       for i in range(cfg.n_layers)]
        self.lm_rows = weights["lm_head"].shape[0]   # (vocab shard) rows of the lm_head

    @property
    def kv_heads_local(self) -> int:
        return self.n_kv_heads

    def attention(self, q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, meta: AttnMeta,
                  kv_scales=(1.0, 1.0)) -> torch.Tensor:
        """``kv_scales``: the layer's (k_scale, v_scale), read only with an fp8 K/V pool (launch constants)."""
        ks, vs = kv_scales
        if meta.kind == "decode":
            return ops.paged_attention_decode(q, kc, vc, meta.block_tables, meta.ctx_lens, self.scale,
                                              meta.num_splits, meta.workspace, groups=meta.groups,
                                              planned=meta.planned, k_scale=ks, v_scale=vs)
        return ops.prefill_attention(q, kc, vc, meta.block_tables, meta.cu_q, meta.start_pos, self.scale,
                                     meta.tile_map, split=meta.prefill_split, k_scale=ks, v_scale=vs)

    def fused_decode_ok(self, ids: torch.Tensor) -> bool:
        """The fused decode path takes up to 16 rows, up to 32 at tp 1 (serving batches: the skinny
        GEMMs' two-row-block launches, csrc/skinny_core.h gemm_tiles; the tensor-parallel epilogues
        stay at 16)."""
        cfg = self.cfg
        rows = 32 if self.tp.size == 1 and not self.force_tp_path else 16
        rows = min(rows, int(os.environ.get("ROUNDTABLE_FUSED_ROWS", rows)))   # A/B knob
        if self.quant in ("fp8", "mxfp4"):
            # tp 1 only, <= 32 rows (two launches of 16); more rows take the unfused path on
            # operands dequantised into scratch (correct, slow)
            if self.tp.size != 1 or self.force_tp_path:
                return False
            rows = min(rows, ops.FP8_MAX_ROWS if self.quant == "fp8" else ops.MXFP4_MAX_ROWS)
        return (ids.is_cuda and 1 <= ids.shape[0] <= rows and self.use_fused
                and cfg.hidden % 32 == 0 and cfg.ffn % 32 == 0 and (cfg.n_heads * cfg.head_dim) % 32 == 0
                and self.lm_rows % 16 == 0)

    use_fused = True
    force_tp_path = False   # tests: run the tensor-parallel fused path at tp=1 (all-reduces are no-ops)
    _dec = None

    # shuffled-only residency: the row-major linears were dropped after shuffling (a knight whose
    # weights do not fit twice, e.g. Llama-3-70B on one GPU); prefill GEMMs rebuild each row-major
    # (gamma-folded) operand in a per-shape scratch buffer with ops.unshuffle_weight
    shuffled_only = False
    _scratch: Optional[Dict[tuple, torch.Tensor]] = None
    # weight quantisation of the decode linears: None | "fp8" (e4m3fn codes + per-row scales,
    # csrc/gemm_skinny_fp8.hip) | "mxfp4" (e2m1 codes + one e8m0 scale byte per 32 k,
    # csrc/gemm_skinny_fp4.hip). Always single-copy: the dequantised row-major operand of the
    # prefill / unfused GEMMs is rebuilt in the same scratch as shuffled-only residency, so every
    # path computes with the SAME weights bf16(code * scale)
    quant: Optional[str] = None

    def quant_width_error(self, quant: str) -> Optional[str]:
        """Why this model's GEMM depths do not fit the k-record of ``quant`` ("fp8": 64 deep,
        "mxfp4": 128 deep) (None: they fit)."""
        cfg = self.cfg
        record = ops.MXFP4_K_RECORD if quant == "mxfp4" else ops.FP8_K_RECORD
        for what, k in (("hidden", cfg.hidden), ("ffn / tp", cfg.ffn // self.tp.size),
                        ("heads x head_dim / tp", self.n_heads * self.head_dim)):
            if k % record:
                return f"{what} = {k} is not a multiple of the {quant} k-record ({record})"
        if self.lm_rows % 16:
            return f"lm_head rows = {self.lm_rows} is not a multiple of 16"
        return None

    def fp8_width_error(self) -> Optional[str]:
        """Why this model's GEMM depths do not fit the fp8 k-record (None: they fit)."""
        return self.quant_width_error("fp8")

    # (name, folded norm, shuffle kwargs) of the linears the fused decode path streams
    # (QK-norm: the qkv GEMM stores plain columns for K2n, so wqkv is not pair-interleaved)
    def _lin_specs(self):
        qkv_kw = {} if self.cfg.qk_norm else {"rope_heads": self.n_heads + self.n_kv_heads, "head_dim": self.head_dim}
        return (("wqkv", "attn_norm", qkv_kw),
                ("wo", None, {}), ("w_gate_up", "ffn_norm", {"swiglu": True}), ("w_down", None, {}))

    def decode_weights(self, drop_originals: bool = False, quant: Optional[str] = None):
        """Fragment-shuffled, norm-folded copies of every linear for the fused decode path (built
        lazily once). Default: +1x weight memory, affordable on 288 GB HBM for 7-8B knights.
        ``drop_originals``: shuffle one linear at a time and free its row-major tensor (peak +1
        tensor), so only ONE copy of the weights stays resident (see :attr:`shuffled_only`).
        ``quant="fp8"``: quantise each linear instead (``name`` -> uint8 codes, ``name_scale`` ->
        fp32 row scales); ``quant="mxfp4"``: ``name`` -> uint8 e2m1 codes ``[N, K/2]``,
        ``name_scale`` -> uint8 block scale bytes ``[N, K/32]``. Both always drop the originals. The
        embedding table stays bf16 (a tied lm_head loses only its own reference)."""
        if self._dec is None:
            if quant not in (None, "none", "fp8", "mxfp4"):
                raise ValueError(f"unknown weight quantisation {quant!r}")
            fp8 = quant in ("fp8", "mxfp4")   # quantised, either type: one copy, no split workspace
            if fp8:
                err = self.quant_width_error(quant)
                if err or self.tp.size != 1:
                    raise ValueError(f"{self.cfg.name}: {quant} weights: {err or 'tensor parallel is not supported'}")
                drop_originals = True
                self.quant = quant

            def shuffle(W, gamma, d, name, **kw):
                if quant == "mxfp4":
                    d[name], d[name + "_scale"] = ops.shuffle_weight_mxfp4(W, gamma, **kw)
                elif fp8:
                    d[name], d[name + "_scale"] = ops.shuffle_weight_fp8(W, gamma, **kw)
                else:
                    d[name] = ops.shuffle_weight(W, gamma, **kw)

            with torch.no_grad():
                layers = []
                for i, lw in enumerate(self.layers):
                    d = {}
                    for name, norm, kw in self._lin_specs():
                        shuffle(lw[name], lw[norm] if norm else None, d, name, **kw)
                        if drop_originals:
                            # drop BOTH references (the per-layer view and the flat dict) now, so the
                            # allocator reuses this tensor's memory for the next shuffle: the load peak
                            # stays one weight copy + one tensor
                            lw[name] = None
                            self.w[f"layers.{i}.{name}"] = None
                    if lw.get("bqkv") is not None:   # Qwen2: the bias the qkv epilogue adds before RoPE
                        d["bqkv"] = ops.rope_bias(lw["bqkv"], self.n_heads, self.n_kv_heads, self.head_dim)
                    if self.cfg.qk_norm:             # Qwen3: the two [head_dim] gammas K2n reads, as they are
                        d["q_norm"], d["k_norm"] = lw["q_norm"], lw["k_norm"]
                    layers.append(d)
                top = {}
                shuffle(self.w["lm_head"], self.w["final_norm"], top, "lm_head")
                lm = top["lm_head"]
                if drop_originals:
                    self.w["lm_head"] = None
                    for k in [k for k in self.w if k.startswith("layers.") and k.split(".", 2)[2] in
                              ("wqkv", "wo", "w_gate_up", "w_down")] + ["lm_head"]:
                        self.w[k] = None
                    self.shuffled_only = True
                    self._scratch = {}
                    if self.device.type == "cuda":
                        torch.cuda.empty_cache()
                # ONE split workspace for every decode GEMM of this model (they run in order on
                # the engine's stream; counters re-arm at the end of each call): split-K for shard
                # shapes with fewer tiles than CUs (tensor parallel), and the balanced launch of
                # gate_up, whose tile count (ffn/16) is rarely a multiple of the CU count
                # (the fp8 / mxfp4 launches have no split forms: no workspace)
                ws = ops.split_workspace(lm.device) if lm.is_cuda and not fp8 else None
                self._dec = {"layers": layers, "split_ws": ws, **top}
        return self._dec

    def _row_major(self, l: Optional[int], name: str) -> torch.Tensor:
        """The row-major operand of a prefill / unfused GEMM: the resident tensor, or (shuffled-only
        residency) the gamma-folded weight unshuffled into a scratch buffer reused per shape."""
        if not self.shuffled_only:
            return self.layers[l][name] if l is not None else self.w[name]
        if l is None:
            d, kw = self._dec, {}
        else:
            d = self._dec["layers"][l]
            kw = next(k for n, _, k in self._lin_specs() if n == name)
        Ws = d[name]
        # (mxfp4 codes hold two k per byte: the operand is [N, K], not the codes' [N, K/2])
        key = (Ws.shape[0], 2 * Ws.shape[1]) if self.quant == "mxfp4" else tuple(Ws.shape)
        buf = self._scratch.get(key)
        if buf is None:
            buf = self._scratch[key] = torch.empty(key, dtype=self.dtype, device=Ws.device)
        if self.quant == "mxfp4":
            return ops.unshuffle_weight_mxfp4(Ws, d[name + "_scale"], out=buf, **kw)
        if self.quant == "fp8":
            return ops.unshuffle_weight_fp8(Ws, d[name + "_scale"], out=buf, **kw)
        return ops.unshuffle_weight(Ws, out=buf, **kw)

    def _norm_w(self, l: Optional[int], name: str) -> torch.Tensor:
        """Norm weight of the unfused path: ones when gamma is folded into the next linear."""
        w = self.layers[l][name] if l is not None else self.w[name]
        if self.shuffled_only:
            ones = self._scratch.get(("ones", w.numel()))
            if ones is None:
                ones = self._scratch[("ones", w.numel())] = torch.ones_like(w)
            return ones
        return w

    def _qkv_fused(self, res, lw, positions, kv, l, meta, eps, **gemm_kw):
        """The fused decode paths' qkv step -> q [B, n_heads, head_dim], K/V written. One launch (the
        GEMM's RoPE / cache epilogue), or with ``cfg.qk_norm`` two: the GEMM stores the plain
        [B, (Hq + 2 Hkv) D] row (EPI_STORE: a workgroup owns 16 of a head's columns, so the per-head sum of
        squares is not available in its epilogue) and K2n normalises, rotates and writes the cache."""
        kc, vc = kv.k_layer(l), kv.v_layer(l)
        ks, vs = kv.scales(l)
        if not self.cfg.qk_norm:
            return ops.skinny_gemm_rope(res, lw["wqkv"], ops.PRO_NORM, positions, self.cos_sin, kc, vc,
                                        meta.slot_mapping, self.n_heads, self.n_kv_heads, self.head_dim, eps,
                                        bias=lw.get("bqkv"), k_scale=ks, v_scale=vs, **gemm_kw)
        qkv = ops.skinny_gemm(res, lw["wqkv"], ops.PRO_NORM, ops.EPI_STORE, eps=eps, **gemm_kw)
        return ops.qk_norm_rope_and_cache(qkv, lw["q_norm"], lw["k_norm"], eps, positions, self.cos_sin, kc, vc,
                                          meta.slot_mapping, self.n_heads, self.n_kv_heads, self.head_dim, ks, vs)

    accepts_hidden = True  # forward(..., hidden=) takes pre-gathered embedding rows (decode_prep)

    def forward_decode_fused(self, ids: torch.Tensor, positions: torch.Tensor, kv, meta: AttnMeta,
                             hidden: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Decode step with every norm / residual / activation fused into the MFMA GEMMs
        (csrc/gemm_skinny.hip): per layer qkv(+RMSNorm, +RoPE/KV-cache write) -> K3 (+ its split
        combine launch) -> o(+residual) -> gate_up(+RMSNorm, SwiGLU) -> down(+residual); no norm /
        rope / reduce kernels. (Folding the combine into the o launch measured slower:
        tools/experiments/combine_o.hip.) With ``cfg.qk_norm`` (Qwen3) the qkv step is two launches,
        qkv(+RMSNorm) storing the plain row and K2n (per-head norm + RoPE + cache write): seven
        launches per layer instead of six (:meth:`_qkv_fused`)."""
        cfg = self.cfg
        eps = cfg.norm_eps
        dec = self.decode_weights()
        # the residual stream is updated in place by every RESID epilogue
        res = hidden if hidden is not None else F.embedding(ids, self.w["embed"]).contiguous()
        B = ids.shape[0]
        sw, SK, ALL = dec["split_ws"], ops.SPLIT_K, ops.SPLIT_K | ops.SPLIT_BALANCE
        for l, lw in enumerate(dec["layers"]):
            # (``*_scale``: fp8 weights' row scales / mxfp4 weights' block scale bytes, absent = bf16)
            kvs = kv.scales(l)       # (k_scale, v_scale): read only with an fp8 K/V pool
            q = self._qkv_fused(res, lw, positions, kv, l, meta, eps, split_ws=sw, split_mode=SK,
                                wscale=lw.get("wqkv_scale"))
            a = self.attention(q, kv.k_layer(l), kv.v_layer(l), meta, kvs)
            ops.skinny_gemm(a.reshape(B, -1), lw["wo"], ops.PRO_PLAIN, ops.EPI_RESID, res=res, split_ws=sw,
                            split_mode=SK, wscale=lw.get("wo_scale"))
            g = ops.skinny_gemm(res, lw["w_gate_up"], ops.PRO_NORM, ops.EPI_SWIGLU, eps=eps, split_ws=sw,
                                split_mode=ALL, wscale=lw.get("w_gate_up_scale"))
            ops.skinny_gemm(g, lw["w_down"], ops.PRO_PLAIN, ops.EPI_RESID, res=res, split_ws=sw, split_mode=SK,
                            wscale=lw.get("w_down_scale"))
        logits = ops.skinny_gemm(res, dec["lm_head"], ops.PRO_NORM, ops.EPI_STORE, eps=eps, split_ws=sw,
                                 split_mode=SK, wscale=dec.get("lm_head_scale"))
        return logits[:, :cfg.vocab]

    def forward_decode_fused_tp(self, ids: torch.Tensor, positions: torch.Tensor, kv, meta: AttnMeta,
                                hidden: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Tensor-parallel fused decode (Megatron split), the same 4 GEMMs per
        layer as tp 1: qkv (RMSNorm + RoPE/KV-cache epilogue) -> K3 -> o -> gate_up (RMSNorm +
        SwiGLU) -> down. o / down are row-parallel: their partial sums are all-reduced over the
        group (C2) and added into the residual stream in place by the same launch — the K9 exchange
        in the GEMM epilogue when the one-shot comm passed its fused self-test, else the GEMM + a
        K9 launch in its residual form (``tp.row_parallel(res=)``). The lm_head is vocab-parallel
        + all-gather (C3). Round 3 instead handed the partial to the next GEMM's NORM_ADD
        prologue, which re-added it in every workgroup: 1-3 us per GEMM at shard shapes
        (profiles/r04/gemm_variants.md). qkv never takes split-K (its seam cost more than the
        48-192 unsplit tiles lose; same table). ``cfg.qk_norm``: qkv is two launches, as at tp 1 (seven
        per layer)."""
        cfg, tp = self.cfg, self.tp
        eps = cfg.norm_eps
        dec = self.decode_weights()
        # the residual stream is updated in place by every row-parallel launch
        res = hidden if hidden is not None else F.embedding(ids, self.w["embed"]).contiguous()
        B = ids.shape[0]
        sk = dict(split_ws=dec["split_ws"], split_mode=ops.SPLIT_K)
        for l, lw in enumerate(dec["layers"]):
            kc, vc = kv.k_layer(l), kv.v_layer(l)
            q = self._qkv_fused(res, lw, positions, kv, l, meta, eps, split_ws=dec["split_ws"], split_mode=0)
            a = self.attention(q, kc, vc, meta, kv.scales(l))
            tp.row_parallel(a.reshape(B, -1), lw["wo"], res=res, **sk)
            g = ops.skinny_gemm(res, lw["w_gate_up"], ops.PRO_NORM, ops.EPI_SWIGLU, eps=eps, **sk)
            tp.row_parallel(g, lw["w_down"], res=res, **sk)
        logits = ops.skinny_gemm(res, dec["lm_head"], ops.PRO_NORM, ops.EPI_STORE, eps=eps, **sk)
        if meta.local_logits:
            return logits
        logits = tp.all_gather_last(logits)
        return logits[:, :cfg.vocab]

    def forward(self, ids: torch.Tensor, positions: torch.Tensor, kv, meta: AttnMeta,
                hidden: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Returns logits [rows, vocab] (all rows for decode, ``meta.last_rows`` for prefill).
        ``hidden``: optional pre-gathered embedding rows (used by the fused decode path only)."""
        if meta.kind == "decode":
            # one attention work plan per decode step, read by all layers' launches
            meta.planned = ops.attn_plan(meta.block_tables, meta.ctx_lens, meta.num_splits, meta.workspace,
                                         self.n_heads, self.n_kv_heads, meta.groups, ids.shape[0])
        if meta.kind == "decode" and self.fused_decode_ok(ids):
            if self.tp.size > 1 or self.force_tp_path:
                return self.forward_decode_fused_tp(ids, positions, kv, meta, hidden)
            return self.forward_decode_fused(ids, positions, kv, meta, hidden)
        cfg, tp = self.cfg, self.tp
        T = ids.shape[0]
        h = F.embedding(ids, self.w["embed"])
        res = None
        for l, lw in enumerate(self.layers):
            if res is None:
                res = h
                x = ops.rms_norm(h, self._norm_w(l, "attn_norm"), cfg.norm_eps)
            else:
                x, res = ops.fused_add_rms_norm(h, res, self._norm_w(l, "attn_norm"), cfg.norm_eps)
            qkv = F.linear(x, self._row_major(l, "wqkv"), lw.get("bqkv"))
            kvs = kv.scales(l)
            if cfg.qk_norm:
                q = ops.qk_norm_rope_and_cache(qkv, lw["q_norm"], lw["k_norm"], cfg.norm_eps, positions, self.cos_sin,
                                               kv.k_layer(l), kv.v_layer(l), meta.slot_mapping, self.n_heads,
                                               self.n_kv_heads, self.head_dim, k_scale=kvs[0], v_scale=kvs[1])
            else:
                q = ops.rope_and_cache(qkv, positions, self.cos_sin, kv.k_layer(l), kv.v_layer(l), meta.slot_mapping,
                                       self.n_heads, self.n_kv_heads, self.head_dim, k_scale=kvs[0], v_scale=kvs[1])
            a = self.attention(q, kv.k_layer(l), kv.v_layer(l), meta, kvs)
            h = tp.all_reduce(F.linear(a.reshape(T, -1), self._row_major(l, "wo")))
            x, res = ops.fused_add_rms_norm(h, res, self._norm_w(l, "ffn_norm"), cfg.norm_eps)
            g = ops.silu_and_mul(F.linear(x, self._row_major(l, "w_gate_up")))
            h = tp.all_reduce(F.linear(g, self._row_major(l, "w_down")))
        if meta.kind == "prefill" and meta.last_rows is not None:
            h = h.index_select(0, meta.last_rows)
            res = res.index_select(0, meta.last_rows)
        x, _ = ops.fused_add_rms_norm(h, res.clone() if not res.is_cuda else res, self._norm_w(None, "final_norm"),
                                      cfg.norm_eps)
        logits = F.linear(x, self._row_major(None, "lm_head"))
        if meta.kind == "decode" and meta.local_logits:
            return logits
        logits = tp.all_gather_last(logits)
        return logits[:, :cfg.vocab]
