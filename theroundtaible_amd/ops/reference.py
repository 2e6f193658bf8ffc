"""Plain-PyTorch reference semantics of every hand-written kernel (the numerics oracle).

These run on CPU (unit tests, the GPT-2 CPU plumbing config) and are what the HIP
kernels in ``csrc/`` are tested against. Layouts are the engine's:

* ``k_cache``: allocated ``[num_blocks, n_kv_heads, block_size, head_dim]``, but each
  ``[block, head]`` block is CHUNK-MAJOR in memory: ``[head_dim/32][block_size][32]`` (round 6,
  csrc/common.h ``kc_elem``: a decode-attention K load instruction then reads whole 128-B lines).
  Index it through :func:`k_blocks` / :func:`k_rows` / :func:`write_k`, never as ``[blk, h, off, :]``.
* ``v_cache``: ``[num_blocks, n_kv_heads, head_dim, block_size]`` (V stored transposed per
  block, so the P.V MFMA B-operand is a contiguous load; see csrc/attention_decode.hip)
* ``slot = block_id * block_size + offset``
* ``cos_sin``: ``[max_pos, head_dim]`` fp32 = ``[cos(pos*f_i) | sin(pos*f_i)]`` over
  ``i < head_dim/2`` (Llama rotate-half convention).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

MASK64 = (1 << 64) - 1


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (y * w.float()).to(x.dtype)


def fused_add_rms_norm(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor,
                       eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    r = (x.float() + residual.float()).to(x.dtype)
    return rms_norm(r, w, eps), r


def layer_norm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float) -> torch.Tensor:
    return torch.nn.functional.layer_norm(x.float(), (x.shape[-1],), w.float(), b.float(), eps).to(x.dtype)


def fused_add_layer_norm(x, residual, w, b, eps):
    r = (x.float() + residual.float()).to(x.dtype)
    return layer_norm(r, w, b, eps), r


def rope_inv_freq(head_dim: int, theta: float, scaling: Optional[tuple] = None) -> Tuple[torch.Tensor, float]:
    """RoPE inverse frequencies (fp64) and the cos / sin magnitude, for the checkpoint's
    ``rope_scaling`` (``models/config.py`` ``ModelConfig.rope_scaling``):

    * ``("linear", factor)``: positions / factor;
    * ``("llama3", factor, low_freq_factor, high_freq_factor, original_max_pos)`` (Llama 3.1 / 3.2):
      wavelengths past ``original / low`` divided by ``factor``, shorter than ``original / high``
      kept, the band between interpolated smoothly;
    * ``("yarn", factor, original_max_pos, beta_fast, beta_slow, attention_factor)`` (YaRN,
      Qwen2.5 long context): per-dimension blend of interpolated / extrapolated frequencies over
      the correction range, cos and sin scaled by ``attention_factor`` (the parser's default:
      0.1 ln(factor) + 1).
    The kernels read the resulting table; nothing else changes."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    mag = 1.0
    if not scaling:
        return inv, mag
    kind = scaling[0]
    if kind == "linear":
        return inv / float(scaling[1]), mag
    if kind == "llama3":
        factor, low_ff, high_ff, orig = (float(v) for v in scaling[1:5])
        wavelen = 2 * math.pi / inv
        low_wl, high_wl = orig / low_ff, orig / high_ff
        out = torch.where(wavelen > low_wl, inv / factor, inv)
        smooth = (orig / wavelen - low_ff) / (high_ff - low_ff)
        mid = (wavelen >= high_wl) & (wavelen <= low_wl)
        return torch.where(mid, (1 - smooth) * out / factor + smooth * out, out), mag
    if kind == "yarn":
        factor, orig, beta_fast, beta_slow, att = (float(v) for v in scaling[1:6])

        def corr_dim(rot):
            return (head_dim * math.log(orig / (rot * 2 * math.pi))) / (2 * math.log(theta))
        low = max(math.floor(corr_dim(beta_fast)), 0)
        high = min(math.ceil(corr_dim(beta_slow)), head_dim - 1)
        if low == high:
            high += 0.001
        ramp = ((torch.arange(head_dim // 2, dtype=torch.float64) - low) / (high - low)).clamp(0, 1)
        extra = 1 - ramp                     # 1: keep the original frequency, 0: interpolate
        out = (inv / factor) * (1 - extra) + inv * extra
        return out, att
    raise ValueError(f"unsupported rope_scaling {scaling!r}")


def rope_cos_sin(max_pos: int, head_dim: int, theta: float, device=None,
                 scaling: Optional[tuple] = None) -> torch.Tensor:
    inv, mag = rope_inv_freq(head_dim, theta, scaling)
    t = torch.arange(max_pos, dtype=torch.float64)
    f = torch.outer(t, inv)
    return torch.cat([f.cos() * mag, f.sin() * mag], dim=-1).float().to(device)


def _rotate(x: torch.Tensor, cs: torch.Tensor) -> torch.Tensor:
    # x [T, H, D] float; cs [T, D]
    d2 = x.shape[-1] // 2
    cos, sin = cs[:, None, :d2], cs[:, None, d2:]
    x1, x2 = x[..., :d2], x[..., d2:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def rope_and_cache(qkv: torch.Tensor, positions: torch.Tensor, cos_sin: Optional[torch.Tensor],
                   k_cache: torch.Tensor, v_cache: torch.Tensor, slot_mapping: torch.Tensor,
                   n_heads: int, n_kv_heads: int, head_dim: int, k_scale: float = 1.0,
                   v_scale: float = 1.0) -> torch.Tensor:
    """Split fused qkv, rotate q/k (if cos_sin given), scatter k/v into the paged cache, return q.
    An fp8 cache (uint8, :func:`kv_fp8_code`) takes the codes of the fp32 k / v under the scales."""
    T = qkv.shape[0]
    q = qkv[:, :n_heads * head_dim].reshape(T, n_heads, head_dim).float()
    k = qkv[:, n_heads * head_dim:(n_heads + n_kv_heads) * head_dim].reshape(T, n_kv_heads, head_dim).float()
    v = qkv[:, (n_heads + n_kv_heads) * head_dim:].reshape(T, n_kv_heads, head_dim)
    if cos_sin is not None:
        cs = cos_sin[positions.long()]
        q = _rotate(q, cs)
        k = _rotate(k, cs)
    bs = k_cache.shape[2]
    slots = slot_mapping.long()
    blk, off = slots // bs, slots % bs
    if is_fp8_cache(k_cache, v_cache):
        write_k_fp8(k_cache, blk, off, kv_fp8_code(k, kv_fp8_inv(k_scale)))
        write_v_fp8(v_cache, blk, off, kv_fp8_code(v.float(), kv_fp8_inv(v_scale)))
        return q.to(qkv.dtype)
    write_k(k_cache, blk, off, k)
    v_cache[blk, :, :, off] = v.to(v_cache.dtype)
    return q.to(qkv.dtype)


def qk_norm_rope_and_cache(qkv: torch.Tensor, q_gamma: torch.Tensor, k_gamma: torch.Tensor, eps: float,
                           positions: torch.Tensor, cos_sin: Optional[torch.Tensor], k_cache: torch.Tensor,
                           v_cache: torch.Tensor, slot_mapping: torch.Tensor, n_heads: int, n_kv_heads: int,
                           head_dim: int, k_scale: float = 1.0, v_scale: float = 1.0) -> torch.Tensor:
    """:func:`rope_and_cache` with a per-head RMSNorm of q and k first (Qwen3's q_norm / k_norm;
    csrc/qk_norm_rope.hip). Per token and head, fp32 throughout: ``ss`` = the sum of the squares of the
    head's ``head_dim`` inputs, ``r = rsqrt(ss / head_dim + eps)``, ``y = x * r * gamma`` (q heads:
    ``q_gamma``, k heads: ``k_gamma``, both ``[head_dim]``; v is not normalised); ``y`` is rotated
    (``cos_sin=None``: not) with NO rounding to bf16 between the norm and the rotation. q leaves as
    ``qkv.dtype``, k and v go to the paged cache as :func:`rope_and_cache` writes them. ``qkv`` is
    only read. Inputs whose sum of squares overflows fp32 (|x| above about 2^60 across a head) are
    outside the contract."""
    T = qkv.shape[0]
    nq, nk = n_heads * head_dim, n_kv_heads * head_dim

    def norm(x, gamma):
        ss = x.pow(2).sum(-1, keepdim=True)
        return x * torch.rsqrt(ss / head_dim + eps) * gamma.float()

    q = norm(qkv[:, :nq].reshape(T, n_heads, head_dim).float(), q_gamma)
    k = norm(qkv[:, nq:nq + nk].reshape(T, n_kv_heads, head_dim).float(), k_gamma)
    v = qkv[:, nq + nk:].reshape(T, n_kv_heads, head_dim)
    if cos_sin is not None:
        cs = cos_sin[positions.long()]
        q = _rotate(q, cs)
        k = _rotate(k, cs)
    bs = k_cache.shape[2]
    slots = slot_mapping.long()
    blk, off = slots // bs, slots % bs
    if is_fp8_cache(k_cache, v_cache):
        write_k_fp8(k_cache, blk, off, kv_fp8_code(k, kv_fp8_inv(k_scale)))
        write_v_fp8(v_cache, blk, off, kv_fp8_code(v.float(), kv_fp8_inv(v_scale)))
        return q.to(qkv.dtype)
    write_k(k_cache, blk, off, k)
    v_cache[blk, :, :, off] = v.to(v_cache.dtype)
    return q.to(qkv.dtype)


# ---- FP8 K/V cache (kv_dtype "fp8"; csrc/kv_fp8_core.h is the same rule on host and device) ----
KV_FP8_MAX = 448.0        # largest finite OCP e4m3fn value
KV_FP8_NAN = 0x7F


def kv_fp8_inv(scale: float) -> torch.Tensor:
    """The fp32 ``1 / scale`` every writer multiplies by (one IEEE fp32 division, as the launchers')."""
    return torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(scale), dtype=torch.float32)


def kv_fp8_code(y: torch.Tensor, inv_scale) -> torch.Tensor:
    """The cache byte (uint8) of fp32 ``y``: e4m3fn round-to-nearest-even of ``clamp(y * inv_scale,
    +-448)`` — one fp32 multiply, the clamp BEFORE the cast (torch's cast gives NaN, not 448, above
    464), +-inf saturates, NaN gives the NaN code 0x7f. The sign bit is kept."""
    inv = torch.as_tensor(inv_scale, dtype=torch.float32).to(y.device)
    t = y.float() * inv
    nan = torch.isnan(t)
    t = torch.where(nan, torch.zeros_like(t), t).clamp(-KV_FP8_MAX, KV_FP8_MAX)
    codes = t.to(torch.float8_e4m3fn).view(torch.uint8)
    return torch.where(nan, torch.full_like(codes, KV_FP8_NAN), codes)


def kv_fp8_value(codes: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """fp32 ``e4m3(code) * scale`` (the convert is exact: every e4m3 value is a bf16 value)."""
    return codes.view(torch.float8_e4m3fn).float() * torch.tensor(float(scale), dtype=torch.float32).to(codes.device)


def is_fp8_cache(k_cache: torch.Tensor, v_cache: Optional[torch.Tensor] = None) -> bool:
    """Whether the caches are the one-byte caches of kv_dtype "fp8"; mixed K/V dtypes are refused."""
    if v_cache is not None and v_cache.dtype != k_cache.dtype:
        raise ValueError(f"mixed K/V cache dtypes: {k_cache.dtype} / {v_cache.dtype}")
    return k_cache.dtype == torch.uint8


def k_blocks_fp8(k_cache: torch.Tensor) -> torch.Tensor:
    """The byte order of an fp8 K cache ``[NB, Hkv, BS, D]`` (csrc/common.h kc8_elem): 64-dim-chunk
    major, ``[NB, Hkv, D/64, BS, 64]``."""
    nb, hkv, bs, d = k_cache.shape
    return k_cache.view(nb, hkv, d // 64, bs, 64)


def v_blocks_fp8(v_cache: torch.Tensor) -> torch.Tensor:
    """The byte order of an fp8 V cache ``[NB, Hkv, D, BS]`` (csrc/common.h vc8_elem):
    ``[NB, Hkv, D/32 e, 16 r, BS/8 g, 2 u, 8 j]`` holds dim ``32e + 16u + r`` of key ``8g + j``."""
    nb, hkv, d, bs = v_cache.shape
    return v_cache.view(nb, hkv, d // 32, 16, bs // 8, 2, 8)


def write_k_fp8(k_cache: torch.Tensor, blk: torch.Tensor, off: torch.Tensor, codes: torch.Tensor) -> None:
    """Store key code rows ``[T, n_kv_heads, head_dim]`` (uint8) at (block, offset) pairs."""
    T, hkv, d = codes.shape
    k_blocks_fp8(k_cache)[blk, :, :, off, :] = codes.reshape(T, hkv, d // 64, 64)


def write_v_fp8(v_cache: torch.Tensor, blk: torch.Tensor, off: torch.Tensor, codes: torch.Tensor) -> None:
    """Store value code rows ``[T, n_kv_heads, head_dim]`` (uint8) at (block, offset) pairs."""
    T, hkv, d = codes.shape
    c = codes.reshape(T, hkv, d // 32, 2, 16).permute(0, 1, 2, 4, 3)          # [T, Hkv, e, r, u]
    v_blocks_fp8(v_cache)[blk, :, :, :, off // 8, :, off % 8] = c


def k_rows_fp8(k_cache: torch.Tensor, blocks: torch.Tensor) -> torch.Tensor:
    """Key code rows of ``blocks`` in order: ``[len(blocks) * block_size, n_kv_heads, head_dim]`` uint8."""
    kb = k_blocks_fp8(k_cache)[blocks]                   # [n, Hkv, D/64, BS, 64]
    n, hkv, c, bs, w = kb.shape
    return kb.permute(0, 3, 1, 2, 4).reshape(n * bs, hkv, c * w)


def v_rows_fp8(v_cache: torch.Tensor, blocks: torch.Tensor) -> torch.Tensor:
    """Value code rows of ``blocks`` in order: ``[len(blocks) * block_size, n_kv_heads, head_dim]`` uint8."""
    vb = v_blocks_fp8(v_cache)[blocks]                   # [n, Hkv, e, r, g, u, j]
    n, hkv, e, r, g, u, j = vb.shape
    return vb.permute(0, 4, 6, 1, 2, 5, 3).reshape(n * g * j, hkv, e * u * r)


def k_blocks(k_cache: torch.Tensor) -> torch.Tensor:
    """The chunk-major view of a K cache: ``[num_blocks, n_kv_heads, head_dim/32, block_size, 32]``."""
    nb, hkv, bs, d = k_cache.shape
    return k_cache.view(nb, hkv, d // 32, bs, 32)


def k_rows(k_cache: torch.Tensor, blocks: torch.Tensor) -> torch.Tensor:
    """Key rows of ``blocks`` in order: ``[len(blocks) * block_size, n_kv_heads, head_dim]``."""
    kb = k_blocks(k_cache)[blocks]                       # [n, Hkv, D/32, BS, 32]
    n, hkv, c, bs, w = kb.shape
    return kb.permute(0, 3, 1, 2, 4).reshape(n * bs, hkv, c * w)


def write_k(k_cache: torch.Tensor, blk: torch.Tensor, off: torch.Tensor, k: torch.Tensor) -> None:
    """Store key rows ``k`` ``[T, n_kv_heads, head_dim]`` at (block, offset) pairs."""
    T, hkv, d = k.shape
    k_blocks(k_cache)[blk, :, :, off, :] = k.reshape(T, hkv, d // 32, 32).to(k_cache.dtype)


def set_k_row(k_cache: torch.Tensor, blk: int, head: int, off: int, row: torch.Tensor) -> None:
    """Store one key row ``[head_dim]`` of one KV head (tests)."""
    k_blocks(k_cache)[blk, head, :, off, :] = row.reshape(-1, 32).to(k_cache.dtype)


def _gather_kv(k_cache, v_cache, block_table, n, k_scale: float = 1.0, v_scale: float = 1.0):
    bs = k_cache.shape[2]
    nblk = (n + bs - 1) // bs
    blocks = block_table[:nblk].long()
    if is_fp8_cache(k_cache, v_cache):
        return (kv_fp8_value(k_rows_fp8(k_cache, blocks)[:n], k_scale),
                kv_fp8_value(v_rows_fp8(v_cache, blocks)[:n], v_scale))
    k = k_rows(k_cache, blocks)[:n]
    v = v_cache[blocks].permute(0, 3, 1, 2).reshape(nblk * bs, v_cache.shape[1], -1)[:n]
    return k.float(), v.float()


def paged_attention_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                           block_tables: torch.Tensor, ctx_lens: torch.Tensor, scale: float,
                           k_scale: float = 1.0, v_scale: float = 1.0) -> torch.Tensor:
    B, Hq, D = q.shape
    Hkv = k_cache.shape[1]
    G = Hq // Hkv
    out = torch.empty_like(q)
    for b in range(B):
        n = int(ctx_lens[b])
        k, v = _gather_kv(k_cache, v_cache, block_tables[b], n, k_scale, v_scale)     # [n, Hkv, D]
        qb = q[b].float().reshape(Hkv, G, D)
        s = torch.einsum("hgd,nhd->hgn", qb, k) * scale
        p = torch.softmax(s, dim=-1)
        o = torch.einsum("hgn,nhd->hgd", p, v)
        out[b] = o.reshape(Hq, D).to(q.dtype)
    return out


def prefill_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                      block_tables: torch.Tensor, cu_q: torch.Tensor, start_pos: torch.Tensor,
                      scale: float, k_scale: float = 1.0, v_scale: float = 1.0) -> torch.Tensor:
    """Varlen causal attention: sequence s has queries cu_q[s]:cu_q[s+1] at absolute positions
    start_pos[s] + i, attending to cached keys [0, start_pos[s] + i]."""
    T, Hq, D = q.shape
    Hkv = k_cache.shape[1]
    G = Hq // Hkv
    out = torch.empty_like(q)
    for s in range(cu_q.shape[0] - 1):
        a, b = int(cu_q[s]), int(cu_q[s + 1])
        if b == a:
            continue
        st = int(start_pos[s])
        n = st + (b - a)
        k, v = _gather_kv(k_cache, v_cache, block_tables[s], n, k_scale, v_scale)
        qs = q[a:b].float().reshape(b - a, Hkv, G, D)
        sc = torch.einsum("thgd,nhd->thgn", qs, k) * scale
        qpos = torch.arange(st, n)[:, None]
        kpos = torch.arange(n)[None, :]
        mask = (kpos <= qpos)[:, None, None, :]
        sc = sc.masked_fill(~mask, float("-inf"))
        p = torch.softmax(sc, dim=-1)
        o = torch.einsum("thgn,nhd->thgd", p, v)
        out[a:b] = o.reshape(b - a, Hq, D).to(q.dtype)
    return out


def rope_row_perm(n_rows: int, rope_heads: int, head_dim: int) -> torch.Tensor:
    """Source row of every output row in the pair-interleaved q/k order of the ROPE epilogue:
    row h*D + 2i <- h*D + i, row h*D + 2i + 1 <- h*D + i + D/2 (rows past the q/k heads: identity)."""
    idx = torch.arange(n_rows)
    r = rope_heads * head_dim
    if r:
        h, p = idx[:r] // head_dim, idx[:r] % head_dim
        idx[:r] = h * head_dim + p // 2 + (p % 2) * (head_dim // 2)
    return idx


def rope_bias(b: torch.Tensor, rope_heads: int, head_dim: int) -> torch.Tensor:
    """A q/k/v bias (natural order) as the ROPE epilogue adds it: fp32, in the pair-interleaved
    column order of the shuffled weight (:func:`rope_row_perm`)."""
    return b.float()[rope_row_perm(b.numel(), rope_heads, head_dim).to(b.device)].contiguous()


def fold_gamma(W, gamma=None, rope_heads: int = 0, head_dim: int = 0):
    """W * gamma[None, :] rounded to W's dtype (the RMSNorm weight folded into the next linear),
    rows optionally permuted for the ROPE epilogue (``rope_heads`` leading heads)."""
    out = W.clone() if gamma is None else (W.float() * gamma.float()[None, :]).to(W.dtype)
    if rope_heads:
        out = out[rope_row_perm(W.shape[0], rope_heads, head_dim)].contiguous()
    return out


FP8_MAX = 448.0   # largest finite OCP e4m3fn value


def quantize_fp8(W, gamma=None, rope_heads: int = 0, head_dim: int = 0):
    """The fp8 weight-only contract (csrc/gemm_skinny_fp8.hip): row-major e4m3fn codes (uint8) and
    one fp32 scale per row of ``wf = fp32(W) * fp32(gamma)`` (no bf16 rounding of the fold):
    ``scale = amax / 448`` (1 for an all-zero row), ``code = e4m3_rne(clamp(wf * (448 / amax),
    +-448))``. The clamp matters: torch's cast gives NaN, not 448, above 464. Rows (and scales)
    permuted for the ROPE epilogue as :func:`fold_gamma`."""
    wf = W.float() if gamma is None else W.float() * gamma.float()[None, :]
    amax = wf.abs().amax(dim=1)
    nz = amax > 0
    # (tensor / tensor: ``448.0 / amax`` would be reciprocal(amax) * 448, two roundings)
    inv = torch.where(nz, torch.full_like(amax, FP8_MAX) / amax, torch.ones_like(amax))
    scale = torch.where(nz, amax / FP8_MAX, torch.ones_like(amax))
    y = (wf * inv[:, None]).clamp(-FP8_MAX, FP8_MAX)
    codes = y.to(torch.float8_e4m3fn).view(torch.uint8)
    if rope_heads:
        perm = rope_row_perm(W.shape[0], rope_heads, head_dim).to(W.device)
        codes, scale = codes[perm].contiguous(), scale[perm].contiguous()
    return codes, scale


def dequantize_fp8(codes, scale):
    """``bf16(code * scale)`` of row-major codes, rows as stored: the weight every fp8 GEMM path
    (fused decode, unfused, prefill) computes with."""
    return (codes.view(torch.float8_e4m3fn).float() * scale.float()[:, None]).to(torch.bfloat16)


MXFP4_BLOCK = 32                                             # k elements per scale byte
MXFP4_MAGNITUDES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # e2m1, code & 7


def mxfp4_scale_byte(amax):
    """The e8m0 scale byte (int32 tensor) of blocks whose largest ``|wf|`` is the fp32 ``amax``:
    ``max(E - 2, 2)``, ``E`` the exponent field of ``amax``."""
    E = (amax.contiguous().view(torch.int32) >> 23) & 0xFF
    return (E - 2).clamp_min(2)


def mxfp4_code(wf, e):
    """The e2m1 code (uint8 tensor, 0..15) of fp32 ``wf`` under the scale byte(s) ``e`` (int32, 2..252,
    broadcast against ``wf``): the rule of :func:`quantize_mxfp4`."""
    wf, e = torch.broadcast_tensors(wf, e)
    inv = ((254 - e) << 23).to(torch.int32).view(torch.float32)          # 2^(127-e), a normal fp32
    y = wf.abs() * inv
    mag = ((y > 0.25).to(torch.uint8) + (y >= 0.75).to(torch.uint8) + (y > 1.25).to(torch.uint8)
           + (y >= 1.75).to(torch.uint8) + (y > 2.5).to(torch.uint8) + (y >= 3.5).to(torch.uint8)
           + (y > 5.0).to(torch.uint8))
    sign = (wf.contiguous().view(torch.int32) < 0).to(torch.uint8)        # the sign BIT: -0.0 counts
    return mag | (sign << 3)


def quantize_mxfp4(W, gamma=None, rope_heads: int = 0, head_dim: int = 0):
    """The MXFP4 weight-only contract (csrc/fp4_core.h, csrc/gemm_skinny_fp4.hip): row-major OCP
    e2m1 codes, two per byte (uint8 ``[N, K/2]``: k = 2j in the low nibble of byte j, 2j + 1 in the
    high), and one e8m0 scale byte per block of 32 consecutive k of a row (uint8 ``[N, K/32]``), of
    ``wf = fp32(W) * fp32(gamma)`` (no bf16 rounding of the fold). Per block: ``E`` = the fp32
    exponent field of the largest ``|wf|``, ``e = max(E - 2, 2)`` (the OCP rule floor(log2 amax) -
    emax(e2m1), floored so 0.5 * 2^(e-127) is a normal bf16; an all-zero block gets e = 2 and zero
    codes), ``y = |wf| / 2^(e-127)`` (exact), code & 7 = the magnitude of {0, .5, 1, 1.5, 2, 3, 4, 6}
    nearest to min(y, 6) with ties to the even code, code bit 3 = the sign bit of ``wf``, always.
    Rows (and their scale bytes) permuted for the ROPE epilogue as :func:`fold_gamma`."""
    N, K = W.shape
    if K % MXFP4_BLOCK:
        raise ValueError(f"mxfp4 blocks are {MXFP4_BLOCK} consecutive k: K = {K} does not divide")
    wf = W.float() if gamma is None else W.float() * gamma.float()[None, :]
    blocks = wf.reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    e = mxfp4_scale_byte(blocks.abs().amax(dim=2))
    c = mxfp4_code(blocks, e[:, :, None]).reshape(N, K // 2, 2)
    codes = (c[:, :, 0] | (c[:, :, 1] << 4)).contiguous()
    scale = e.to(torch.uint8)
    if rope_heads:
        perm = rope_row_perm(N, rope_heads, head_dim).to(W.device)
        codes, scale = codes[perm].contiguous(), scale[perm].contiguous()
    return codes, scale


def dequantize_mxfp4(codes, scale):
    """``bf16(value(code) * 2^(e-127))`` (exact) of row-major :func:`quantize_mxfp4` codes and scale
    bytes, rows as stored: the weight every mxfp4 GEMM path (fused decode, unfused, prefill)
    computes with. Any codes and scale bytes in 2..252 are valid, not only the quantiser's."""
    N, K2 = codes.shape
    c = torch.stack([codes & 15, codes >> 4], dim=2).reshape(N, 2 * K2).long()
    table = torch.tensor(MXFP4_MAGNITUDES + tuple(-m for m in MXFP4_MAGNITUDES), dtype=torch.float32,
                         device=codes.device)
    two_e = (scale.to(torch.int32) << 23).view(torch.float32)            # 2^(e-127)
    v = table[c].reshape(N, -1, MXFP4_BLOCK) * two_e.reshape(N, -1)[:, :, None]
    return v.reshape(N, 2 * K2).to(torch.bfloat16)


def skinny_gemm(x, Wf, pro=0, epi=0, res=None, eps=1e-5, x2=None, xout=None):
    """Semantics of csrc/gemm_skinny.hip on the (gamma-folded, row-major) weight ``Wf``:
    y = rsqrt(mean(x^2) + eps)[:, None] * (x @ Wf^T) for the NORM prologue; NORM_ADD (pro=2)
    first forms x = bf16(x + x2) and stores it to ``xout``."""
    if pro == 2:
        x = (x.float() + x2.float()).to(x.dtype)
        if xout is not None:
            xout.copy_(x)
    M, K = x.shape
    xf = x.float()
    y = xf @ Wf.float().t()
    if pro in (1, 2):
        y = y * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    if epi == 2:
        n = Wf.shape[0] // 2
        return (torch.nn.functional.silu(y[:, :n]) * y[:, n:]).to(x.dtype)
    if epi == 1:
        res.copy_((y + res.float()).to(res.dtype))
        return None
    if epi == 3:
        return y  # fp32 pre-rope projection (see skinny_gemm_rope)
    return y.to(x.dtype)


def skinny_gemm_rope(x, Wp, pro, positions, cos_sin, k_cache, v_cache, slots, n_heads, n_kv_heads, head_dim,
                     eps=1e-5, x2=None, xout=None, bias=None, k_scale: float = 1.0, v_scale: float = 1.0):
    """ROPE-epilogue semantics: fp32 projection on the pair-permuted weight (+ the fp32 bias in
    the same column order, :func:`rope_bias`), columns restored to natural order, then RoPE +
    paged K/V scatter with no bf16 rounding in between."""
    y = skinny_gemm(x, Wp, pro, 3, None, eps, x2, xout)
    if bias is not None:
        y = y + bias.float()[None, :]
    perm = rope_row_perm(Wp.shape[0], n_heads + n_kv_heads, head_dim)
    qkv = torch.empty_like(y)
    qkv[:, perm] = y
    q = rope_and_cache(qkv, positions, cos_sin, k_cache, v_cache, slots, n_heads, n_kv_heads, head_dim, k_scale,
                       v_scale)
    return q.to(x.dtype)


def silu_and_mul(x: torch.Tensor) -> torch.Tensor:
    d = x.shape[-1] // 2
    xf = x.float()
    return (torch.nn.functional.silu(xf[..., :d]) * xf[..., d:]).to(x.dtype)


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.gelu(x.float(), approximate="tanh").to(x.dtype)


# ---- sampling -----------------------------------------------------------------------------
# Counter-based RNG shared bit-for-bit with csrc/sampling.hip: u = mix(seed, offset, idx).

def _mix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def uniform_tensor(seed: int, offset: int, n: int) -> torch.Tensor:
    """u in (0,1) for token indices 0..n-1 (vectorized with int64 wraparound arithmetic)."""
    key = _mix64((seed & MASK64) ^ _mix64(offset & MASK64))
    idx = torch.arange(n, dtype=torch.int64)
    z = _mix_t(idx + _to_signed(key))
    # top 24 bits -> (0,1)
    hi = (z >> 40) & 0xFFFFFF
    return (hi.double() + 0.5) / float(1 << 24)


def _to_signed(x: int) -> int:
    return x - (1 << 64) if x >= (1 << 63) else x


def _mix_t(z: torch.Tensor) -> torch.Tensor:
    def mul(a, c):
        return a * _to_signed(c)  # int64 multiply wraps mod 2^64

    def srl(a, s):  # logical right shift on int64
        return (a >> s) & ((1 << (64 - s)) - 1)

    z = z + _to_signed(0x9E3779B97F4A7C15)
    z = mul(z ^ srl(z, 30), 0xBF58476D1CE4E5B9)
    z = mul(z ^ srl(z, 27), 0x94D049BB133111EB)
    return z ^ srl(z, 31)


def sample(logits: torch.Tensor, temperature: torch.Tensor, top_p: torch.Tensor, top_k: torch.Tensor,
           seeds: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """Greedy when temperature <= 0; else Gumbel-max over the top-k ∩ top-p set.

    Row b's noise is a pure function of (seeds[b], offsets[b], token index); the engine
    passes each knight's token position as its offset, so a knight's sample stream is
    independent of batching, graph replay and round mode."""
    B, V = logits.shape
    out = torch.empty(B, dtype=torch.int64)
    for b in range(B):
        l = logits[b].float()
        t = float(temperature[b])
        if t <= 0:
            out[b] = int(torch.argmax(l))
            continue
        z = (l - l.max()) / t
        allowed = torch.ones(V, dtype=torch.bool)
        k = int(top_k[b])
        if 0 < k < V:
            kth = torch.topk(z, k).values[-1]
            allowed &= z >= kth
        p = float(top_p[b])
        if p < 1.0:
            w = torch.where(allowed, torch.exp(z.double()), torch.zeros((), dtype=torch.float64))
            srt, _ = torch.sort(w, descending=True)
            cs = torch.cumsum(srt, 0)
            cut = int(torch.searchsorted(cs, p * cs[-1]).clamp(max=V - 1))
            thr = srt[cut]
            allowed &= w >= thr
        u = uniform_tensor(int(seeds[b]), int(offsets[b]), V)
        g = -torch.log(-torch.log(u))
        score = torch.where(allowed, z.double() + g, torch.full((), float("-inf"), dtype=torch.float64))
        out[b] = int(torch.argmax(score))
    return out


def decode_prep(slots, offsets, res, ids, positions, block_tables, embed, block_size):
    """Semantics of csrc/decode_step.hip::decode_prep (in place). A position past the block
    table (only after a turn's last step; that slot is never written) maps into block 0."""
    pos = positions.long()
    bi = pos // block_size
    inside = bi < block_tables.shape[1]
    blk = block_tables.long().gather(1, torch.where(inside, bi, 0).unsqueeze(1)).squeeze(1)
    blk = torch.where(inside, blk, 0)
    slots[:len(pos)] = blk * block_size + pos % block_size
    offsets[:len(pos)] = pos + 1
    tok = ids.long().clamp(0, embed.shape[0] - 1)
    res.copy_(embed[tok].to(res.dtype))


def decode_advance(out, ids, positions, ctx_lens, step, nxt, prep=None):
    """Semantics of csrc/decode_step.hip::decode_advance (in place); with prep operands
    (slots, offsets, res, block_tables, embed, block_size) it then runs decode_prep."""
    st = int(step.item())
    if st < out.shape[0]:
        out[st] = nxt
    ids.copy_(nxt)
    positions.add_(1)
    ctx_lens.add_(1)
    step.add_(1)
    if prep is not None:
        slots, offsets, res, bt, embed, bs = prep
        decode_prep(slots, offsets, res, ids, positions, bt, embed, bs)


PAGING_GUARD_CODES = {1: "ctx_len outside [1, max_blocks*block_size]", 2: "block-table entry outside the KV pool",
                      4: "K/V write slot does not match block_tables[pos // block_size]",
                      8: "ctx_len != position + 1"}


def paging_guard(block_tables, ctx_lens, positions, slots, err, num_blocks, block_size):
    """Semantics of csrc/decode_step.hip::paging_guard (err[0] |= violation bits, in place)."""
    code = 0
    maxb = block_tables.shape[1]
    for b in range(ctx_lens.numel()):
        ctx = int(ctx_lens[b])
        if ctx < 1 or ctx > maxb * block_size:
            code |= 1
        nt = min((max(ctx, 0) + block_size - 1) // block_size, maxb)
        row = block_tables[b, :nt]
        if nt and (int(row.min()) < 0 or int(row.max()) >= num_blocks):
            code |= 2
        if positions is not None:
            pos = int(positions[b])
            if pos + 1 != ctx:
                code |= 8
            if slots is not None and pos >= 0 and pos // block_size < maxb:
                want = int(block_tables[b, pos // block_size]) * block_size + pos % block_size
                if int(slots[b]) != want:
                    code |= 4
    err[0] = int(err[0]) | code


# ---- logit processors (csrc/logit_proc.hip) -------------------------------------------------------

LOGIT_PROC_WINDOW = 2048      # both windows (repetition set, counted reply) reach back this far
LOGIT_PROC_MAX_BIAS = 300     # OpenAI's limit on logit_bias entries


def logit_proc_history(proc, b: int, out=None, step=None) -> Tuple[list, int]:
    """Row b's token history ``S = hist[b, :hist_len[b]] ++ out[0:step, b]`` (time order) and the
    index in S at which the reply starts."""
    n_host = min(max(int(proc.hist_len[b]), 0), proc.hist.shape[1])
    S = [int(t) for t in proc.hist[b, :n_host].tolist()]
    if step is not None and out is not None:
        n_dev = min(max(int(step.reshape(-1)[0]), 0), out.shape[0])
        S += [int(t) for t in out[:n_dev, b].tolist()]
    return S, min(max(int(proc.reply_from[b]), 0), n_host)


def apply_logit_processors(logits: torch.Tensor, proc, out=None, step=None) -> torch.Tensor:
    """Semantics of csrc/logit_proc.hip (in place, fp32 on the stored logit, one rounding on the
    store): bias, then the repetition penalty over the last ``last_n`` tokens of S, then frequency
    and presence over the reply part of S; both windows capped at LOGIT_PROC_WINDOW. Tokens
    outside [0, V) are ignored, -inf stays -inf, unnamed elements and neutral rows are not touched."""
    B, V = logits.shape
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)       # noqa: E731
    for b in range(B):
        rp, pp, fp = f32(proc.rp[b]), f32(proc.pp[b]), f32(proc.fp[b])
        nb = min(max(int(proc.bias_n[b]), 0), proc.bias_tok.shape[1], LOGIT_PROC_MAX_BIAS)
        ln = int(proc.last_n[b])
        n_rep = 0 if (float(rp) == 1.0 or ln == 0) else (LOGIT_PROC_WINDOW if ln < 0 else min(ln, LOGIT_PROC_WINDOW))
        counted = float(pp) != 0.0 or float(fp) != 0.0
        if n_rep == 0 and not counted and nb == 0:
            continue
        S, rf = logit_proc_history(proc, b, out, step)
        bias = {}
        for j in range(nb):                      # a token named twice: the last entry holds
            bias[int(proc.bias_tok[b, j])] = f32(proc.bias_val[b, j])
        rep = set(S[len(S) - min(n_rep, len(S)):])
        count: dict = {}
        if counted:
            for t in S[rf:][-LOGIT_PROC_WINDOW:]:
                count[t] = count.get(t, 0) + 1
        for t in set(bias) | rep | set(count):
            if not 0 <= t < V:
                continue
            l = logits[b, t].float()
            if float(l) == float("-inf"):
                continue
            if t in bias:
                l = l + bias[t]
            if t in rep:
                l = l / rp if float(l) > 0 else l * rp
            c = count.get(t, 0)
            if c > 0:
                l = l - fp * f32(c)
                l = l - pp
            logits[b, t] = l.to(logits.dtype)
    return logits


# ---- logprobs (csrc/logprobs.hip) ------------------------------------------------------------------

MAX_TOP_LOGPROBS = 20                 # alternatives a row can ask for (OpenAI's limit)
LOGPROB_CHUNK = 4096                  # csrc/logprobs_plan.h: elements per chunk, at most 64 chunks
LOGPROB_WS_ROW = 64 * 44              # workspace words per row, whatever V is


def logprob_step(ids=None, out=None, step=None):
    """-> (chosen tokens, record row) of a logprob call, or None when the graph form's step is
    outside the record: ``ids`` form -> row 0; ``(out, step)`` form -> the token K6 just recorded,
    ``out[step - 1]``, and row ``step - 1``."""
    if step is not None and out is not None:
        s = int(step.reshape(-1)[0]) - 1
        return (out[s], s) if 0 <= s < out.shape[0] else None
    return ids, 0


def token_logprobs(logits: torch.Tensor, lp, ids=None, out=None, step=None):
    """Semantics of csrc/logprobs.hip in fp32: per row with ``n_top >= 0``, on the logits as sampled
    from (l = the stored value as fp32), ``lse = logsumexp(l)``, the chosen token's ``l - lse``
    (NaN for an id outside [0, V)) and the ``n_top`` largest l, value descending then token id
    ascending (a stable sort), each with ``l - lse``; entries past min(n_top, V): id -1, lp -inf.
    Rows with ``n_top < 0`` write nothing. The logits are only read."""
    at = logprob_step(ids, out, step)
    if at is None:
        return lp
    toks, rec = at
    B, V = logits.shape
    for b in range(B):
        nt = min(int(lp.n_top[b]), MAX_TOP_LOGPROBS)
        if nt < 0:
            continue
        l = logits[b].detach().float() + 0.0        # -0.0 ties with +0.0
        lse = torch.logsumexp(l, 0)
        vals, idx = torch.sort(l, descending=True, stable=True)      # stable: equal values keep id order
        k = min(nt, V)
        lp.top_id[rec, b] = -1
        lp.top_lp[rec, b] = float("-inf")
        lp.top_id[rec, b, :k] = idx[:k].to(torch.int32)
        lp.top_lp[rec, b, :k] = vals[:k] - lse
        t = int(toks[b])
        lp.tok_lp[rec, b] = (l[t] - lse) if 0 <= t < V else float("nan")
    return lp


# ---- grammar mask (csrc/grammar_mask.hip, walk: csrc/grammar_core.h) -------------------------------

GRAMMAR_MAX_DEPTH = 32                # engine/grammar.py holds the same limits (tests hold them together)
GRAMMAR_MAX_STATES = 4096
GRAMMAR_MAX_CLASSES = 64
GRAMMAR_MAX_TABLE = 65536
GRAMMAR_TOKEN_BYTE_CAP = 128
GRAMMAR_MAX_STOPS = 8
GRAMMAR_Q_FIN, GRAMMAR_Q_DEAD = -1, -2
GRAMMAR_META = 8                      # ints per row: active, n_states, n_classes, pop obj / arr / empty, n_stop, pad


class GrammarRow:
    """Row ``b`` of a GrammarMask's device-format operands, read back to the host."""

    def __init__(self, gm, b: int):
        m = [int(x) for x in gm.meta[b].tolist()]
        self.active = m[0] != 0
        self.ns = min(max(m[1], 0), gm.accept.shape[1])
        self.nc = min(max(m[2], 0), GRAMMAR_MAX_CLASSES)
        if self.ns * self.nc > gm.tab.shape[1]:
            self.ns = 0
        self.pops = m[3:6]
        n_stop = min(max(m[6], 0), GRAMMAR_MAX_STOPS)
        self.stops = [int(x) for x in gm.stops[b, :n_stop].tolist()]
        self.cls = gm.cls[b].cpu().long()
        self.tab = gm.tab[b, :self.ns * self.nc].cpu().long() & 0xFFFF
        self.accept = gm.accept[b].cpu()
        self.tok_off = gm.tok_off.cpu().long()
        self.tok_bytes = gm.tok_bytes.cpu()


def grammar_walk(row: GrammarRow, st: Tuple[int, int, int], data) -> Tuple[int, int, int]:
    """grammar_core.h ``walk``: advance (q, depth, stack) over bytes; (Q_DEAD, 0, 0) when it dies."""
    q, depth, stack = st
    dead = (GRAMMAR_Q_DEAD, 0, 0)
    if q < 0:
        return st
    if q >= row.ns or not 0 <= depth <= GRAMMAR_MAX_DEPTH:
        return dead
    for byte in data:
        c = int(row.cls[int(byte)])
        if c >= row.nc:
            return dead
        e = int(row.tab[q * row.nc + c])
        if e == 0xFFFF:
            return dead
        act = e & 3
        if act == 3:
            if depth == 0:
                return dead
            depth -= 1
            stack &= ~(1 << depth)
            q = row.pops[2 if depth == 0 else (stack >> (depth - 1)) & 1]
        else:
            if act:
                if depth == GRAMMAR_MAX_DEPTH:
                    return dead
                stack |= (act - 1) << depth
                depth += 1
            q = e >> 2
        if not 0 <= q < row.ns:
            return dead
    return (q, depth, stack)


def grammar_token_bytes(row: GrammarRow, tok: int, V: int) -> bytes:
    """The bytes of ``tok``; empty for an id outside [0, V), a zero-length token or one over the byte cap."""
    if not 0 <= tok < V:
        return b""
    a, b = int(row.tok_off[tok]), int(row.tok_off[tok + 1])
    if a < 0 or b <= a or b > row.tok_bytes.numel() or b - a > GRAMMAR_TOKEN_BYTE_CAP:
        return b""
    return bytes(row.tok_bytes[a:b].tolist())


def grammar_advance(row: GrammarRow, st, tok: int, V: int):
    """grammar_core.h ``advance``: FIN / DEAD stay, a stop id gives FIN, an unusable token or a dead walk DEAD."""
    if st[0] < 0:
        return st
    if tok in row.stops:
        return (GRAMMAR_Q_FIN, 0, 0)
    data = grammar_token_bytes(row, tok, V)
    return grammar_walk(row, st, data) if data else (GRAMMAR_Q_DEAD, 0, 0)


def grammar_walk_all(row: GrammarRow, st, V: int):
    """Every token of [0, V) walked at once from state ``st``, one byte position per iteration:
    ``(alive bool [V], q, depth, stack int64 [V])``, the last three meaningful where ``alive``. A state
    outside the table walks nothing."""
    q0, d0, s0 = st
    if q0 >= row.ns or not 0 <= d0 <= GRAMMAR_MAX_DEPTH:
        q0 = GRAMMAR_Q_DEAD
    q = torch.full((V,), q0, dtype=torch.int64)
    depth = torch.full((V,), d0, dtype=torch.int64)
    stack = torch.full((V,), s0 & 0xFFFFFFFF, dtype=torch.int64)
    alive = torch.zeros(V, dtype=torch.bool)
    if q0 >= 0:
        lo, hi = row.tok_off[:V], row.tok_off[1:V + 1]
        lens = hi - lo
        alive = (lens > 0) & (lens <= GRAMMAR_TOKEN_BYTE_CAP) & (lo >= 0) & (hi <= row.tok_bytes.numel())
        lens = torch.where(alive, lens, torch.zeros_like(lens))
        pops = torch.tensor(row.pops, dtype=torch.int64)
        one = torch.ones(1, dtype=torch.int64)
        for p in range(int(lens.max()) if V else 0):
            idx = torch.nonzero(alive & (lens > p)).squeeze(1)
            if idx.numel() == 0:
                break
            c = row.cls[row.tok_bytes[lo[idx] + p].long()]
            e = row.tab[(q[idx] * row.nc + c).clamp(max=max(row.tab.numel() - 1, 0))] if row.tab.numel() else c * 0 + 0xFFFF
            dead = (c >= row.nc) | (e == 0xFFFF)
            act = e & 3
            pop, push = act == 3, (act == 1) | (act == 2)
            d, s = depth[idx], stack[idx]
            dead |= (pop & (d == 0)) | (push & (d == GRAMMAR_MAX_DEPTH))
            d_pop = (d - 1).clamp(min=0)
            s_pop = s & ~torch.bitwise_left_shift(one, d_pop)
            top = torch.where(d_pop == 0, torch.full_like(d, 2), torch.bitwise_right_shift(s_pop, (d_pop - 1).clamp(min=0)) & 1)
            s_push = s | torch.bitwise_left_shift((act - 1).clamp(min=0), d.clamp(max=GRAMMAR_MAX_DEPTH - 1))
            qn = torch.where(pop, pops[top], e >> 2)
            dead |= (qn < 0) | (qn >= row.ns)
            keep = ~dead
            alive[idx[dead]] = False
            ik = idx[keep]
            q[ik] = qn[keep]
            depth[ik] = torch.where(pop, d_pop, torch.where(push, d + 1, d))[keep]
            stack[ik] = torch.where(pop, s_pop, torch.where(push, s_push, s))[keep]
    return alive, q, depth, stack


def grammar_allowed(row: GrammarRow, st, V: int) -> torch.Tensor:
    """bool [V]: the tokens the mask kernel leaves untouched at state ``st``."""
    allowed = grammar_walk_all(row, st, V)[0]
    q0 = st[0] if st[0] < row.ns and 0 <= st[1] <= GRAMMAR_MAX_DEPTH else GRAMMAR_Q_DEAD
    stop_ok = q0 < 0 or bool(row.accept[q0])
    for t in row.stops:
        if 0 <= t < V:
            allowed[t] = stop_ok
    return allowed


def grammar_step_state(gm, row: GrammarRow, b: int, V: int, out=None, step=None):
    """Row b's current state as the kernel derives it, and the slot to store it to (None: no store)."""
    s = int(step.reshape(-1)[0]) if step is not None and out is not None else 0
    if s < 0 or s > (out.shape[0] if out is not None else 0):
        return (GRAMMAR_Q_DEAD, 0, 0), None
    src = [int(x) for x in gm.state[(s - 1) & 1 if s > 0 else 0, b].tolist()]
    st = (src[0], src[1], src[2] & 0xFFFFFFFF)
    if s == 0:
        return st, None
    return grammar_advance(row, st, int(out[s - 1, b]), V), s & 1


def apply_grammar_mask(logits: torch.Tensor, gm, out=None, step=None) -> torch.Tensor:
    """Semantics of csrc/grammar_mask.hip (in place): per row with a grammar, -inf over every token that
    is not allowed at the row's current state; allowed elements, rows without a grammar and columns
    past V are not written. ``step=None``: the state is slot 0 of ``gm.state``. With the graph's ``out``
    and ``step = s > 0`` the state is slot ``(s - 1) & 1`` advanced over ``out[s - 1, b]``, stored to slot
    ``s & 1``."""
    B, V = logits.shape
    for b in range(B):
        if int(gm.meta[b, 0]) == 0:
            continue
        row = GrammarRow(gm, b)
        st, slot = grammar_step_state(gm, row, b, V, out, step)
        if slot is not None:
            stack = st[2] - (1 << 32) if st[2] >= (1 << 31) else st[2]
            gm.state[slot, b] = torch.tensor([st[0], st[1], stack, 0], dtype=torch.int32).to(gm.state.device)
        allowed = grammar_allowed(row, st, V)
        logits[b, :V][~allowed.to(logits.device)] = float("-inf")
    return logits


# ---- budgeted grammar mask (csrc/grammar_budget.hip; the bound and the rule: csrc/grammar_core.h) ------

GRAMMAR_NEED_INF16 = 0xFFFF           # engine/grammar.py holds the same three
GRAMMAR_NEED_INF = 1 << 30
GRAMMAR_BUDGET_FREE = 1 << 29


def grammar_need(row: GrammarRow, c_acc: torch.Tensor, c_pop: torch.Tensor, q, depth, stack) -> torch.Tensor:
    """grammar_core.h ``need`` over vectors of live states (int64): ``c_acc[q]`` at depth 0, else ``c_pop[q]``
    + one ``c_pop[pop target]`` per stack level below the top + ``c_acc[pop_empty]``; ``NEED_INF`` where a
    16-bit entry it reads says none."""
    inf16 = GRAMMAR_NEED_INF16
    pobj, parr, pempty = row.pops
    ent = lambda arr, p: int(arr[p]) if 0 <= p < row.ns else inf16        # noqa: E731
    qc = q.clamp(0, max(row.ns - 1, 0))
    below = torch.bitwise_left_shift(torch.ones_like(depth), (depth - 1).clamp(min=0)) - 1
    m = stack & below
    ones = torch.zeros_like(depth)
    for i in range(GRAMMAR_MAX_DEPTH):
        ones += torch.bitwise_right_shift(m, i) & 1
    zeros = (depth - 1 - ones).clamp(min=0)
    a, p = c_acc[qc], c_pop[qc]
    eo, ea, ee = ent(c_pop, pobj), ent(c_pop, parr), ent(c_acc, pempty)
    deep = p + zeros * eo + ones * ea + ee
    bad = (p == inf16) | (ee == inf16) | ((zeros > 0) & (eo == inf16)) | ((ones > 0) & (ea == inf16))
    deep = torch.where(bad, torch.full_like(deep, GRAMMAR_NEED_INF), deep)
    flat = torch.where(a == inf16, torch.full_like(a, GRAMMAR_NEED_INF), a)
    return torch.where(depth == 0, flat, deep)


def grammar_allowed_budget(row: GrammarRow, st, V: int, r: int, c_acc: torch.Tensor, c_pop: torch.Tensor):
    """bool [V] under the budget rule with ``r`` tokens left, and the need after each allowed token
    (int64 [V], meaningful where a non-stop token is allowed). The all-live flags and ``need_cap`` only
    let the kernel skip work: they are not read here."""
    if r <= 0 and st[0] >= 0:
        st = (GRAMMAR_Q_DEAD, 0, 0)
    walks = row.__dict__.setdefault("_walks", {})      # a reply revisits few states (free text, a string's inside)
    if (st, V) not in walks and len(walks) >= 64:
        walks.clear()
    alive, q, depth, stack = walks.get((st, V)) or walks.setdefault((st, V), grammar_walk_all(row, st, V))
    alive = alive.clone()
    need = torch.zeros(V, dtype=torch.int64)
    if bool(alive.any()):
        idx = torch.nonzero(alive).squeeze(1)
        need[idx] = grammar_need(row, c_acc, c_pop, q[idx], depth[idx], stack[idx])
        alive &= need <= r - 2
    q0 = st[0] if st[0] < row.ns and 0 <= st[1] <= GRAMMAR_MAX_DEPTH else GRAMMAR_Q_DEAD
    stop_ok = q0 < 0 or bool(row.accept[q0])
    for t in row.stops:
        if 0 <= t < V:
            alive[t] = stop_ok
    return alive, need


def apply_grammar_mask_budget(logits: torch.Tensor, gm, out=None, step=None) -> torch.Tensor:
    """Semantics of csrc/grammar_budget.hip (in place): :func:`apply_grammar_mask` where, with
    ``r = gm.budget[b] - step`` tokens left, a non-stop token must also leave ``need(state after it) <= r - 2``
    and ``r <= 0`` allows stop ids only. State hand-over as in :func:`apply_grammar_mask`."""
    B, V = logits.shape
    s = int(step.reshape(-1)[0]) if step is not None and out is not None else 0
    for b in range(B):
        if int(gm.meta[b, 0]) == 0:
            continue
        rows = gm.__dict__.setdefault("_ref_rows", {})      # a row's host copy, until the next fill()
        row = rows.get(b) or rows.setdefault(b, GrammarRow(gm, b))
        st, slot = grammar_step_state(gm, row, b, V, out, step)
        if slot is not None:
            stack = st[2] - (1 << 32) if st[2] >= (1 << 31) else st[2]
            gm.state[slot, b] = torch.tensor([st[0], st[1], stack, 0], dtype=torch.int32).to(gm.state.device)
        r = max(-1, min(int(gm.budget[b]) - max(s, 0), GRAMMAR_BUDGET_FREE))
        allowed, _ = grammar_allowed_budget(row, st, V, r, gm.need[0, b].cpu().long() & 0xFFFF,
                                            gm.need[1, b].cpu().long() & 0xFFFF)
        logits[b, :V][~allowed.to(logits.device)] = float("-inf")
    return logits
