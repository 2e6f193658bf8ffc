"""fp64 oracle of the elementwise kernels (csrc/norm.hip, activation.hip, rope_cache.hip), the logit
processors, the logprobs and the attention kernels.

Plain PyTorch on the CPU. Every operation returns the UNROUNDED fp64 result ``e`` and the
magnitude ``mag`` its tolerance is built from; :func:`assert_within` compares a kernel's bf16
output with ``e``. The tolerances are derived, not tuned: a correct fp32 kernel differs from the
fp64 result by one bf16 rounding (``bf16_ulp(e)``; correct rounding alone costs half of it) plus
fp32 error (unit round-off 2^-24) that is far below a bf16 ulp except where terms cancel:

* norms: ``bf16_ulp(e) + 2^-14 * mag`` with ``mag = |xhat * w| + |b|`` (RMS: ``|e|``). The slack
  covers the fp32 error of the mean entering ``x - mean``, amplified by mean / sigma <= 2^8 for
  bf16 data: 2^-24 * 2^8 = 2^-16, with 4x margin.
* ``silu_and_mul``: ``bf16_ulp(e) + 2^-14 * |e| + 2^-100``. The fast exp loses about
  |x| * log2(e) * 2^-24 <= 2^-17 relative for |x| <= 88; the floor covers exp overflow / flush
  (|silu| < 1e-36 there) and subnormals.
* ``gelu_tanh``: ``bf16_ulp(e) + 2^-21 * |x| + 2^-100``. ``1 + tanh`` carries about 2^-22
  absolute error, times 0.5 |x|, with 4x margin (it cancels for x in [-7, -4]).
* RoPE: ``bf16_ulp(e) + 2^-20 * (|x1 c| + |x2 s|)``, the two products of the output at hand.
* logit processors (csrc/logit_proc.hip; bf16 or fp32 logits): ``ulp(e) + 2^-22 * mag`` in the
  storage dtype's ulp, with ``mag`` the largest magnitude any step of ``l + bias``, ``/ rp`` or ``* rp``,
  ``- fp * c``, ``- pp`` reaches: the kernel rounds the product and each of the four steps to fp32,
  five roundings of at most 2^-24 * mag each (a division by rp < 1 scales the error carried so
  far by 1 / rp, and the step's magnitude with it), so 2^-22 * mag bounds their sum with 1.6x margin.
* logprobs (csrc/logprobs.hip): ``2^-21 * (1 + |l| + |lse|)`` on fp32 values, ids exactly; the
  slack is measured, not derived: 4x the fp32 CPU reference's own worst error (see LOGPROB_SLACK).
* attention (csrc/attn_core.h, attention_decode.hip, attention_prefill32.hip, attention_prefill.hip):
  ``bf16_ulp(e) + ((0 if p_exact else 2^-8) + ATTN_SLACK) * A`` with ``A = sum_j w_j |v_j[d]|``, the
  softmax-weighted mean of |V| in the output's dimension. All three kernels round every p to bf16
  for the P.V MFMA (``pack2``, round to nearest) and add the UNROUNDED p into the row sum, so only
  the numerator ``sum_j p_j v_j`` carries the rounding: at most ``u * sum_j p_j |v_j|``, after the
  division ``u * A``, with u the unit round-off of bf16. bf16 has 8 significant bits, so u = 2^-8:
  half a spacing, 2^-9 of the binade's lower end, is 2^-8 of a p just above a power of two and
  2^-9 only of one just below the next. (A first version of this bound took 2^-9. Exact arithmetic
  refutes it: 31 keys, weights 0.605 / 0.370 on values of opposite sign, A = 0.5208; bf16 P with
  every other step in fp64 is off by 1.0885e-3 = 1.07 * 2^-9 * A -- the peaky decode case (28, 4,
  128), row of 31 keys, head 9, dim 47.) The denominator carries no rounding and storing the result
  costs one bf16 rounding, ``bf16_ulp(e)``. The 32x32 prefill kernel's deferred rescale
  (RESCALE_LOG2 = 8) lets p reach 2^8 times the running-max term; the rounding stays relative.
  ``p_exact`` holds for the census inputs only: every live score is exactly 0, so every p is
  exp2(0) = 1 under any running max, split or merge, and the row sums are exact integers. The rest
  (fp32 scores, exp2, fp32 sums, merges) is ATTN_SLACK, measured like LOGPROB_SLACK: 4x the fp32
  CPU reference's own worst ``|o32 - e| / A`` (ATTN_REF_WORST), never against the kernels. Every
  output element is compared.

The input builders of the CPU emulation test and the GPU test live here too, so both see the
same bits.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

GELU_K0 = 0.7978845608028654     # sqrt(2 / pi), csrc/activation.hip
GELU_K1 = 0.044715

NORM_SLACK = 2.0 ** -14
SILU_SLACK = 2.0 ** -14
GELU_SLACK = 2.0 ** -21
ROPE_SLACK = 2.0 ** -20
FLOOR = 2.0 ** -100


def bf16_ulp(t: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 at |t|: 2^(floor(log2 |t|) - 7), |t| clamped below at 2^-126 (fp64).
    Non-finite entries get the spacing of 1 (they are compared by position, not by distance)."""
    a = t.double().abs()
    a = torch.where(torch.isfinite(a), a, torch.ones_like(a)).clamp_min(2.0 ** -126)
    _, ex = torch.frexp(a)                      # a = m * 2^ex, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(a), ex - 8)


def fp32_ulp(t: torch.Tensor) -> torch.Tensor:
    """Spacing of fp32 at |t| (2^-16 of :func:`bf16_ulp`: 23 explicit mantissa bits against 7)."""
    return bf16_ulp(t) * 2.0 ** -16


def storage_ulp(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    return {torch.bfloat16: bf16_ulp, torch.float32: fp32_ulp}[dtype](t)


def assert_within(got: torch.Tensor, e: torch.Tensor, tol: torch.Tensor, what: str = "",
                  dtype: torch.dtype = torch.bfloat16) -> float:
    """``|got - e| <= tol`` wherever ``e`` rounds to a finite bf16 (``dtype``: the storage type);
    NaN, +inf and -inf of ``got`` sit exactly where ``e`` rounded to it has them. Returns the worst
    error / tolerance."""
    assert got.dtype == dtype, f"{what}: output is {got.dtype}, not {dtype}"
    g = got.detach().cpu().double().reshape(-1)
    e = e.double().reshape(-1)
    tol = tol.double().reshape(-1)
    assert g.shape == e.shape == tol.shape, f"{what}: shapes {tuple(g.shape)} {tuple(e.shape)} {tuple(tol.shape)}"
    if g.numel() == 0:
        return 0.0
    eb = e.float().to(dtype).double()
    for name, fn in (("NaN", torch.isnan), ("+inf", lambda v: v == float("inf")),
                     ("-inf", lambda v: v == float("-inf"))):
        bad = fn(g) != fn(eb)
        assert not bool(bad.any()), (f"{what}: {name} mismatch at {int(bad.nonzero()[0])} of {g.numel()} "
                                     f"({int(bad.sum())} places): got {g[bad][0].item()}, oracle {e[bad][0].item()}")
    fin = torch.isfinite(eb)
    if not bool(fin.any()):
        return 0.0
    ratio = (g[fin] - e[fin]).abs() / tol[fin]
    worst = int(ratio.argmax())
    r = float(ratio[worst])
    assert r <= 1.0, (f"{what}: error / tolerance = {r:.3f} at finite element {worst}: got {g[fin][worst].item()!r}, "
                      f"oracle {e[fin][worst].item()!r}, tol {tol[fin][worst].item():.3g}; "
                      f"{int((ratio > 1).sum())} of {ratio.numel()} outside")
    return r


# ---- fp64 operations ------------------------------------------------------------------------

def add_residual(x: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """The stored residual ``bf16(x + r)`` (fp32 sum, as ops/reference.py)."""
    return (x.float() + r.float()).to(x.dtype)


def rms_norm(x, w, eps) -> Tuple[torch.Tensor, torch.Tensor]:
    xd = x.double()
    e = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps) * w.double()
    return e, e.abs()


def layer_norm(x, w, b, eps) -> Tuple[torch.Tensor, torch.Tensor]:
    xd = x.double()
    d = xd - xd.mean(-1, keepdim=True)
    xw = d * torch.rsqrt(d.pow(2).mean(-1, keepdim=True) + eps) * w.double()
    bd = b.double().expand_as(xw)
    return xw + bd, xw.abs() + bd.abs()


def fused_add_rms_norm(x, r, w, eps):
    """-> (e, mag, residual)"""
    res = add_residual(x, r)
    return (*rms_norm(res, w, eps), res)


def fused_add_layer_norm(x, r, w, b, eps):
    res = add_residual(x, r)
    return (*layer_norm(res, w, b, eps), res)


def norm_tol(e, mag):
    return bf16_ulp(e) + NORM_SLACK * mag


def silu_and_mul(x) -> Tuple[torch.Tensor, torch.Tensor]:
    i = x.shape[-1] // 2
    g, u = x[..., :i].double(), x[..., i:].double()
    e = g / (1.0 + torch.exp(-g)) * u
    return e, e.abs()


def silu_tol(e, mag):
    return bf16_ulp(e) + SILU_SLACK * mag + FLOOR


def gelu_tanh(x) -> Tuple[torch.Tensor, torch.Tensor]:
    xd = x.double()
    e = 0.5 * xd * (1.0 + torch.tanh(GELU_K0 * (xd + GELU_K1 * xd * xd * xd)))
    return e, xd.abs()


def gelu_tol(e, mag):
    return bf16_ulp(e) + GELU_SLACK * mag + FLOOR


def rope(x: torch.Tensor, cs: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rotate-half RoPE of ``x`` [T, heads, D] by the fp32 table rows ``cs`` [T, D] = cos | sin
    (None: no rotation). ``mag``: |x1 c| + |x2 s| for the first half, |x2 c| + |x1 s| for the second."""
    xd = x.double()
    if cs is None:
        return xd, xd.abs()
    h = x.shape[-1] // 2
    c, s = cs.double()[:, None, :h], cs.double()[:, None, h:]
    x1, x2 = xd[..., :h], xd[..., h:]
    e = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    mag = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], dim=-1)
    return e, mag


def rope_tol(e, mag):
    return bf16_ulp(e) + ROPE_SLACK * mag


# ---- per-head QK-norm + RoPE (csrc/qk_norm_rope.hip) --------------------------------------------------
# Tolerance of one output element: qk_norm_tol(e, mag) = bf16_ulp(e) + QKNORM_SLACK * mag, with ``mag`` =
# :func:`rope`'s magnitude of the NORMALISED values (|y1 c| + |y2 s|; |y| without a rotation). The bf16
# ulp is the one rounding of the store. The rest (the fp32 sum of squares, rsqrt, two multiplies, the
# rotation) is QKNORM_SLACK, measured like LOGPROB_SLACK and ATTN_SLACK: the worst |o32 - e| / mag of the
# fp32 CPU REFERENCE (ops/reference.py qk_norm_rope_and_cache on fp32 copies of the bf16 inputs, so its
# output carries no bf16 rounding) over every input of QKNORM_SHAPES x QKNORM_T x QKNORM_EPS x {rope,
# no rope} (QKNORM_REF_WORST; tests/test_qk_norm_cpu.py recomputes and prints it), times 4 for the
# device's rsqrt, its butterfly summation order and its fused multiply-adds, rounded up to a power of
# two. It is not tuned against the kernel.
QKNORM_REF_WORST = 3.04e-7       # measured (tests/test_qk_norm_cpu.py::test_reference_vs_oracle_and_worst_is_recorded
#                                  prints it: 3.039e-7 at (12, 12, 64), T = 3, eps 1e-5, with RoPE)
QKNORM_SLACK = 2.0 ** -19        # 4 * 3.04e-7 = 1.22e-6 <= 2^-19 = 1.91e-6
QKNORM_SHAPES = ((32, 8, 128), (4, 1, 128), (16, 8, 128), (40, 8, 128), (12, 12, 64), (1, 1, 64))    # hq, hkv, D
QKNORM_T = (1, 3, 37)
QKNORM_EPS = (1e-6, 1e-5)


def qk_norm_rope(x: torch.Tensor, gq: torch.Tensor, gk: torch.Tensor, eps: float, cs: Optional[torch.Tensor],
                 n_q: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp64 ``rope(rms_norm(x))`` of the q and k heads ``x`` [T, n_q + n_k, D] (q heads first; ``n_q``
    None: every head is a q head): each head normalised over D with ``eps`` and scaled by ``gq`` [D]
    (heads < n_q) or ``gk`` [D], then rotated by the fp32 table rows ``cs`` [T, D] (None: no rotation).
    -> ``(e, mag)``, ``mag`` = :func:`rope`'s magnitude of the normalised values."""
    n_q = x.shape[1] if n_q is None else n_q
    yq, _ = rms_norm(x[:, :n_q], gq, eps)
    yk, _ = rms_norm(x[:, n_q:], gk, eps)
    return rope(torch.cat([yq, yk], dim=1), cs)


def qk_norm_tol(e, mag):
    return bf16_ulp(e) + QKNORM_SLACK * mag


def qk_norm_gammas(D: int, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16 ``(q_gamma, k_gamma)`` [D] around 1 with negative, zero and large entries in both (64 for q;
    -16 for k, which keeps every normalised key of the test inputs below the fp8 cache's 448 x 0.37)."""
    g = _gen(7100 + D + seed)
    gq, gk = _randn((D,), g, 0.3, 1.0), _randn((D,), g, 0.3, 1.0)
    gq[1], gq[D // 2 + 2], gq[5], gq[D - 1] = -0.75, 0.0, 64.0, -1.5
    gk[0], gk[3], gk[D // 2], gk[D - 2] = 0.0, -16.0, 2.5, -0.5
    return gq, gk


def qk_norm_case(hq: int, hkv: int, D: int, T: int, seed: int = 0):
    """:func:`rope_case` with the fixed rows of the QK-norm tests written into ``qkv`` (token 0, and
    token T - 1 where T > 1): q head 0 holds one element 2^15 among values near 2^-8, the last k head is
    all zero (its output is exactly zero under any eps > 0), and in the last token q head ``hq - 1``
    sits at |x| = 2^60 (the sum of squares stays finite in fp32: 128 * 2^120 = 2^127; larger inputs are
    outside the contract); in the one-head, one-token case that row replaces the first.
    -> (qkv, positions, slots, k_cache, v_cache)."""
    qkv, pos, slots, kc, vc = rope_case(hq, hkv, D, T, seed)
    g = _gen(7200 + seed + 13 * hq + 7 * hkv + D + 1000 * T)
    rows = qkv.view(T, hq + 2 * hkv, D)
    small = _randn((D,), g, 2.0 ** -8)
    small[D // 3] = 2.0 ** 15
    rows[0, 0] = small
    rows[0, hq + hkv - 1] = 0.0
    sign = torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0)
    rows[T - 1, hq - 1] = (sign * 2.0 ** 60).to(torch.bfloat16)
    return qkv, pos, slots, kc, vc


LOGIT_PROC_SLACK = 2.0 ** -22
LOGIT_PROC_WINDOW = 2048
LOGIT_PROC_MAX_BIAS = 300


def apply_logit_processors(logits: torch.Tensor, proc, out=None, step=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp64 twin of ops.apply_logit_processors, not in place: ``(e, mag, named)`` with ``e`` the
    unrounded processed logits [B, V], ``mag`` the tolerance magnitude and ``named`` the mask of the
    elements a history token or a bias entry names in a non-neutral row (every other element must
    keep its bits). Written apart from ops/reference.py: whole-row bincounts, not a per-token loop."""
    B, V = logits.shape
    e = logits.detach().cpu().double().clone()
    mag = e.abs()
    mag = torch.where(torch.isfinite(mag), mag, torch.zeros_like(mag))
    named = torch.zeros(B, V, dtype=torch.bool)
    W = LOGIT_PROC_WINDOW
    for b in range(B):
        rp, pp, fp = (float(t[b]) for t in (proc.rp, proc.pp, proc.fp))
        last_n = int(proc.last_n[b])
        n_bias = min(max(int(proc.bias_n[b]), 0), proc.bias_tok.shape[1], LOGIT_PROC_MAX_BIAS)
        rep_n = 0 if rp == 1.0 else (W if last_n < 0 else min(last_n, W))
        if rep_n == 0 and pp == 0.0 and fp == 0.0 and n_bias == 0:
            continue
        n_host = min(max(int(proc.hist_len[b]), 0), proc.hist.shape[1])
        S = proc.hist[b, :n_host].cpu().long()
        if step is not None and out is not None:
            S = torch.cat([S, out[:min(max(int(step.reshape(-1)[0]), 0), out.shape[0]), b].cpu().long()])
        start = min(max(int(proc.reply_from[b]), 0), n_host)

        def hits(part: torch.Tensor) -> torch.Tensor:
            part = part[(part >= 0) & (part < V)]
            return torch.bincount(part, minlength=V).double()

        in_rep = hits(S[max(len(S) - rep_n, 0):]) > 0 if rep_n > 0 else torch.zeros(V, dtype=torch.bool)
        reply = S[start:]
        cnt = hits(reply[max(len(reply) - W, 0):]) if (pp != 0.0 or fp != 0.0) else torch.zeros(V, dtype=torch.float64)
        bias = torch.zeros(V, dtype=torch.float64)
        has_bias = torch.zeros(V, dtype=torch.bool)
        for j in range(n_bias):                 # in order: a token named twice keeps its last entry
            t = int(proc.bias_tok[b, j])
            if 0 <= t < V:
                bias[t] = float(proc.bias_val[b, j])
                has_bias[t] = True
        l = e[b]
        live = l != float("-inf")
        m = mag[b]
        l1 = torch.where(has_bias & live, l + bias, l)
        m = torch.maximum(m, torch.where(live, l1.abs(), m))
        l2 = torch.where(in_rep & live, torch.where(l1 > 0, l1 / rp, l1 * rp), l1)
        if rp > 0:      # dividing by rp < 1 scales the error carried so far by 1 / rp
            m = torch.where(in_rep & live, torch.maximum(l2.abs(), m * max(1.0, 1.0 / rp)), m)
        l3 = torch.where((cnt > 0) & live, l2 - fp * cnt, l2)
        m = torch.maximum(m, torch.where(live, torch.maximum(l3.abs(), (fp * cnt).abs()), m))
        l4 = torch.where((cnt > 0) & live, l3 - pp, l3)
        m = torch.maximum(m, torch.where(live, l4.abs(), m))
        e[b], mag[b] = l4, m
        named[b] = has_bias | in_rep | (cnt > 0)
    return e, mag, named


def logit_proc_tol(e, mag, dtype: torch.dtype = torch.bfloat16):
    return storage_ulp(e, dtype) + LOGIT_PROC_SLACK * mag


# ---- input builders (shared by tests/test_elementwise_oracle_cpu.py and test_elementwise_gpu.py) --

NORM_H = (8, 72, 520, 896, 5120, 8192, 8200, 12288, 16384, 32760, 32768)
NORM_ROWS = (1, 5)
OFFSET_ROWS = ((100.0, 2.0), (3000.0, 16.0), (-20000.0, 100.0))      # LayerNorm: mean, sigma


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _randn(shape, g, scale=1.0, offset=0.0) -> torch.Tensor:
    return (offset + scale * torch.randn(*shape, generator=g)).to(torch.bfloat16)


def norm_params(H: int, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Random bf16 weight and bias."""
    g = _gen(1000 + 7 * H + seed)
    return _randn((H,), g), _randn((H,), g)


def _outliers(shape, g) -> torch.Tensor:
    x = torch.randn(*shape, generator=g)
    H = shape[-1]
    flat = x.reshape(-1, H)
    for row in flat:                                # three elements per row at +-2000
        idx = torch.randperm(H, generator=g)[:3]
        row[idx] = torch.tensor([2000.0, -2000.0, 2000.0])
    return flat.reshape(shape).to(torch.bfloat16)


def norm_cases(shape, ln: bool, add: bool, seed: int = 0) -> List[Tuple[str, torch.Tensor, Optional[torch.Tensor], float]]:
    """The value regimes of one norm case: ``(name, x, r, eps)`` with bf16 ``x`` (and ``r`` for the
    fused-add forms, else None) of ``shape`` = [..., H]."""
    shape = tuple(shape)
    g = _gen(17 + 31 * shape[-1] + 3 * len(shape) + shape[0] + 101 * seed + (1 << 20) * ln + (1 << 21) * add)
    n01 = lambda scale=1.0, offset=0.0: _randn(shape, g, scale, offset)   # noqa: E731
    second = (lambda *a: n01(*a)) if add else (lambda *a: None)
    const = lambda v: torch.full(shape, v, dtype=torch.bfloat16)           # noqa: E731
    cases = [
        ("n01", n01(), second(), 1e-5),
        ("tiny_eps1e-5", n01(2.0 ** -10), second(2.0 ** -10), 1e-5),
        ("tiny_eps1e-6", n01(2.0 ** -10), second(2.0 ** -10), 1e-6),
        ("outliers", _outliers(shape, g), second(), 1e-5),
        ("const3", const(1.0) if add else const(3.0), const(2.0) if add else None, 1e-5),
    ]
    if ln:
        for mean, sigma in OFFSET_ROWS:
            cases.append((f"offset{mean:g}+-{sigma:g}", n01(sigma, mean), second(), 1e-5))
    if add:
        x = n01(50.0)
        r = (-x.float() + torch.randn(*shape, generator=g) * 2.0 ** -4).to(torch.bfloat16)
        cases.append(("cancel", x, r, 1e-5))
    return cases


def finite_bf16_table() -> torch.Tensor:
    """All 65280 finite bf16 bit patterns, in bit order."""
    bits = torch.arange(1 << 16, dtype=torch.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    return bits.to(torch.int16).view(torch.bfloat16)


def tiled_table(n: int, seed: int) -> torch.Tensor:
    """``n`` values: a random permutation of :func:`finite_bf16_table`, tiled."""
    t = finite_bf16_table()
    t = t[torch.randperm(t.numel(), generator=_gen(seed))]
    return t.repeat((n + t.numel() - 1) // t.numel())[:n].clone()


def silu_up_random(shape, seed: int) -> torch.Tensor:
    """``bf16(4 N(0,1))`` with a few entries at +-3e38 (products that overflow bf16)."""
    g = _gen(seed)
    up = _randn(shape, g, 4.0).reshape(-1)
    idx = torch.randperm(up.numel(), generator=g)[:6]
    up[idx] = torch.tensor([3e38, -3e38, 3e38, -3e38, 3e38, -3e38]).to(torch.bfloat16)[:idx.numel()]
    return up.reshape(shape)


def silu_inputs() -> Dict[str, torch.Tensor]:
    """``x`` = [gate | up] of every silu_and_mul case but the grid-stride one."""
    gate = finite_bf16_table().reshape(255, 256)
    g = _gen(5)
    return {
        "table_up1": torch.cat([gate, torch.ones_like(gate)], dim=-1),
        "table_uprand": torch.cat([gate, silu_up_random(gate.shape, 6)], dim=-1),
        "rows1_I8": _randn((1, 16), g, 2.0),
        "rows3_I24": _randn((3, 48), g, 2.0),
    }


SILU_STRIDE_SHAPE = (129, 32776)           # rows, I: 528513 chunks > 2048 * 256 threads
GELU_STRIDE_N = 8 * (524288 + 3)


def silu_stride_input() -> torch.Tensor:
    """Gate: the tiled table. Up: :func:`silu_up_random`, as in the table case: the tolerance's
    2^-100 floor stands for |silu(gate)| < 1e-36 (fp32 exp overflow returns -0 there) times an
    |up| of ordinary size; under an |up| ~ 1e38 of the table that flush is an error of order 1
    in ANY fp32 evaluation of silu(gate) * up, the PyTorch one included."""
    rows, i = SILU_STRIDE_SHAPE
    gate = tiled_table(rows * i, 7).reshape(rows, i)
    return torch.cat([gate, silu_up_random(gate.shape, 10)], dim=-1)


def gelu_inputs() -> Dict[str, torch.Tensor]:
    return {"table": finite_bf16_table().reshape(8160, 8), "n8": _randn((8,), _gen(8), 2.0)}


def gelu_stride_input() -> torch.Tensor:
    return tiled_table(GELU_STRIDE_N, 9)


ROPE_SHAPES = ((1, 1, 32), (32, 8, 128), (12, 12, 64), (8, 1, 128), (4, 2, 256))    # hq, hkv, D
ROPE_T = (1, 37)
ROPE_MAX_POS = 2048
ROPE_THETA = 500000.0
ROPE_BLOCKS, ROPE_BS = 3, 32


def rope_case(hq: int, hkv: int, D: int, T: int, seed: int = 0, first_pos: int = 0):
    """-> qkv [T, (hq + 2 hkv) D] bf16, positions [T] (0 and max_pos - 1 among them when T > 1;
    ``first_pos`` for token 0), distinct slots [T] in a cache of ROPE_BLOCKS blocks, and the
    initial k_cache [NB, hkv, BS, D] / v_cache [NB, hkv, D, BS]."""
    g = _gen(40 + seed + 13 * hq + 7 * hkv + D + 1000 * T)
    qkv = _randn((T, (hq + 2 * hkv) * D), g)
    pos = torch.randint(0, ROPE_MAX_POS, (T,), generator=g)
    pos[0] = first_pos
    if T > 1:
        pos[T - 1] = ROPE_MAX_POS - 1
    slots = torch.randperm(ROPE_BLOCKS * ROPE_BS, generator=g)[:T]
    kc = _randn((ROPE_BLOCKS, hkv, ROPE_BS, D), g)
    vc = _randn((ROPE_BLOCKS, hkv, D, ROPE_BS), g)
    return qkv, pos, slots, kc, vc


# logit processors: B = 3 rows (neutral, penalties only, penalties + 300 biases)
LOGIT_PROC_V = (32064, 1003)
LOGIT_PROC_HIST = (0, 1, 2048, 3000)        # the last exceeds the window: truncated
LOGIT_PROC_STEPS = (0, 1, 2500)
LOGIT_PROC_OUT_ROWS = 2600
LOGIT_PROC_HIST_CAP = 3008


def logit_proc_case(V: int, dtype: torch.dtype, n_hist: int, step: int, seed: int = 0):
    """-> (logits [3, V] of ``dtype``, proc (CPU ops.LogitProc), out [2600, 3] int64, step [1] int64).

    History and bias tokens come from a pool ``{t, t + 4096, t + 8192}`` (one home slot of the
    kernel's 4096-slot table each triple: probing) with duplicates and ids outside [0, V) mixed in;
    the logits at pool tokens cycle through negative, zero, positive and -inf. Row 0 is neutral."""
    from . import LogitProc
    g = _gen(9000 + 13 * V + 7 * n_hist + step + 1000003 * seed + (dtype == torch.float32))
    B = 3
    base = torch.randperm(min(V, 4096), generator=g)[:96]
    pool = torch.cat([base, base + 4096, base + 8192, torch.tensor([-1, -7, V, V + 7, 2 ** 31 - 1])])

    def draw(n):
        return pool[torch.randint(0, pool.numel(), (n,), generator=g)]

    logits = (4.0 * torch.randn(B, V, generator=g)).to(dtype)
    inside = pool[(pool >= 0) & (pool < V)]
    vals = torch.tensor([-3.5, 0.0, 2.75, float("-inf"), -0.0, 7.0, -11.0, 0.40625]).to(dtype)
    logits[:, inside] = vals[torch.arange(inside.numel()) % vals.numel()].expand(B, -1)
    proc = LogitProc(B, "cpu", hist_cap=LOGIT_PROC_HIST_CAP)
    for b in range(B):
        proc.hist[b, :n_hist] = draw(n_hist).to(torch.int32)
    proc.hist_len.fill_(n_hist)
    proc.reply_from.copy_(torch.tensor([0, n_hist // 2, n_hist // 3], dtype=torch.int32))
    k = (n_hist + step) % 4
    proc.rp.copy_(torch.tensor([1.0, 1.3, 0.8]))
    proc.last_n.copy_(torch.tensor([64, (64, -1, 0, 5000)[k], (-1, 1, 64, 2048)[k]], dtype=torch.int32))
    proc.pp.copy_(torch.tensor([0.0, 0.4, -0.3]))
    proc.fp.copy_(torch.tensor([0.0, 0.15, 0.07]))
    nb = LOGIT_PROC_MAX_BIAS
    n_in = min(100, inside.numel())             # the rest random: a token named twice keeps its last entry
    proc.bias_tok[2, :nb] = torch.cat([inside[:n_in], torch.randperm(V, generator=g)[:nb - 2 - n_in],
                                       torch.tensor([-1, V])]).to(torch.int32)
    proc.bias_val[2, :nb] = (200.0 * torch.rand(nb, generator=g) - 100.0)
    proc.bias_val[2, :4] = torch.tensor([-100.0, 100.0, 0.0, 1.5])
    proc.bias_n[2] = nb
    out = torch.stack([draw(LOGIT_PROC_OUT_ROWS) for _ in range(B)], dim=1).to(torch.int64).contiguous()
    return logits, proc, out, torch.tensor([step], dtype=torch.int64)


# ---- logprobs (csrc/logprobs.hip) ------------------------------------------------------------------
# Tolerance: |lp - e| <= LOGPROB_SLACK * (1 + |l| + |lse|), lp compared as fp32, l the token's stored
# logit. lp = l - lse is one fp32 subtraction of two numbers of those magnitudes, after an lse whose
# error is a few fp32 roundings of |lse| plus the relative error of the sum. The slack is the worst
# ratio of the fp32 REFERENCE (ops/reference.py, torch logsumexp) against this oracle over every case
# of LOGPROB_KINDS x LOGPROB_V x {bf16, fp32} plus the B = 32 case, measured on the CPU
# (LOGPROB_REF_WORST), times 4 for the device's expf / logf and its chunked summation order, rounded
# up to a power of two. It is not tuned against the kernel.
LOGPROB_REF_WORST = 8.11e-8      # measured (tests/test_logprobs_cpu.py::test_reference_vs_oracle prints it)
LOGPROB_SLACK = 2.0 ** -21       # 4 * 8.11e-8 = 3.24e-7 <= 2^-21 = 4.77e-7
MAX_TOP_LOGPROBS = 20
LOGPROB_V = (19, 1003, 4096, 4097, 32064)
LOGPROB_V_BIG = 152064            # 38 chunks, one case
LOGPROB_KINDS = ("random", "equal", "levels8", "top_one_chunk", "top_spread", "last", "big80", "banned300",
                 "finite5")


def token_logprobs(logits: torch.Tensor, n_top, toks):
    """fp64 twin of ops.token_logprobs on the exact stored values: ``(tok_lp [B], top_id [B, 20],
    top_lp [B, 20], lse [B], l_tok [B], l_top [B, 20])``. Ids are decided exactly (a stable sort of
    the stored values: value descending, token id ascending). Rows with ``n_top < 0`` hold NaN / -2
    (never compared). Written apart from ops/reference.py: max-shifted sum in fp64, not logsumexp."""
    B, V = logits.shape
    K = MAX_TOP_LOGPROBS
    tok_lp = torch.full((B,), float("nan"), dtype=torch.float64)
    top_id = torch.full((B, K), -2, dtype=torch.int64)
    top_lp = torch.full((B, K), float("nan"), dtype=torch.float64)
    lse = torch.full((B,), float("nan"), dtype=torch.float64)
    l_tok = torch.zeros(B, dtype=torch.float64)
    l_top = torch.zeros(B, K, dtype=torch.float64)
    for b in range(B):
        nt = min(int(n_top[b]), K)
        if nt < 0:
            continue
        l = logits[b].detach().cpu().double() + 0.0
        m = l.max()
        lse[b] = m + torch.log(torch.exp(l - m).sum()) if bool(torch.isfinite(m)) else m
        order = torch.argsort(l, descending=True, stable=True)
        k = min(nt, V)
        top_id[b] = -1
        top_lp[b] = float("-inf")
        top_id[b, :k] = order[:k]
        l_top[b, :k] = torch.where(torch.isfinite(l[order[:k]]), l[order[:k]], torch.zeros(k, dtype=torch.float64))
        top_lp[b, :k] = l[order[:k]] - lse[b]
        t = int(toks[b])
        if 0 <= t < V:
            tok_lp[b] = l[t] - lse[b]
            l_tok[b] = l[t] if bool(torch.isfinite(l[t])) else 0.0
    return tok_lp, top_id, top_lp, lse, l_tok, l_top


def logprob_tol(e, l_tok, lse, dtype: torch.dtype = torch.bfloat16):
    """Tolerance of the logprob ``e`` of a token whose stored logit is ``l_tok`` (0 where it is not
    finite: such an ``e`` is -inf or NaN and compared by position). The same for both dtypes: the
    stored logit is exact in fp32 either way."""
    return LOGPROB_SLACK * (1.0 + l_tok.double().abs() + lse.double().abs()) * torch.ones_like(e, dtype=torch.float64)


def logprob_ntop(B: int) -> torch.Tensor:
    """B = 3: (-1, 0, 20); larger batches mix off rows, 0, 1, 5, 19 and 20."""
    mix = (-1, 0, 20, 5, 1, 19, -1, 20, 7)
    return torch.tensor([mix[b % len(mix)] for b in range(B)], dtype=torch.int32)


def logprob_case(V: int, dtype: torch.dtype, kind: str, seed: int = 0, B: int = 3, ld: Optional[int] = None):
    """-> (logits [B, V] of ``dtype``, a view of NaN-padded rows ``ld`` apart when ``ld`` is given;
    n_top [B] int32; toks [B] int64, the chosen tokens). Kinds: LOGPROB_KINDS.

    random: N(0, 4). equal: one value everywhere. levels8: 8 bf16 levels, ties at every cut.
    top_one_chunk / top_spread: the 20 largest inside the last chunk / one per chunk, round robin.
    last: the maximum and the chosen token at V - 1. big80: around +-80 (fp32 overflows without the
    max subtraction). banned300: 300 tokens at -inf, the chosen one among them. finite5: 5 finite.
    With B > 3 two chosen ids lie outside [0, V)."""
    g = _gen(77000 + 31 * V + 1009 * seed + 7 * LOGPROB_KINDS.index(kind) + (dtype == torch.float32) + 13 * B)
    CH = 4096
    x = 4.0 * torch.randn(B, V, generator=g)
    toks = torch.randint(0, V, (B,), generator=g)
    if kind == "equal":
        x = torch.full((B, V), 1.625)
    elif kind == "levels8":
        lv = torch.tensor([-3.5, -0.0, 0.0, 2.75, 2.765625, -11.0, 0.40625, 2.75])
        x = lv[torch.randint(0, 8, (B, V), generator=g)]
    elif kind in ("top_one_chunk", "top_spread"):
        nch = (V + CH - 1) // CH
        for b in range(B):
            if kind == "top_one_chunk":
                lo = (nch - 1) * CH
                pos = lo + torch.randperm(V - lo, generator=g)[:MAX_TOP_LOGPROBS]
            else:
                pos = torch.tensor([(j % nch) * CH + int(torch.randint(0, min(CH, V - (j % nch) * CH), (1,),
                                                                         generator=g)) for j in range(MAX_TOP_LOGPROBS)])
            x[b, pos] = 30.0 + 0.5 * torch.arange(pos.numel(), dtype=torch.float32)
    elif kind == "last":
        x[:, V - 1] = 40.0
        toks[:] = V - 1
    elif kind == "big80":
        x = 80.0 * torch.sign(torch.randn(B, V, generator=g)) + torch.randn(B, V, generator=g)
    elif kind == "banned300":
        for b in range(B):
            ban = torch.randperm(V, generator=g)[:min(300, V - 1)]
            x[b, ban] = float("-inf")
            toks[b] = ban[0]
    elif kind == "finite5":
        for b in range(B):
            keep = torch.randperm(V, generator=g)[:5]
            v = x[b, keep].clone()
            x[b] = float("-inf")
            x[b, keep] = v
    if B > 3:
        toks[B - 1], toks[B - 2] = V, -1
    n_top = logprob_ntop(B)
    if ld is None:
        return x.to(dtype), n_top, toks.to(torch.int64)
    store = torch.full((B, ld), float("nan"), dtype=dtype)
    store[:, :V] = x.to(dtype)
    return store[:, :V], n_top, toks.to(torch.int64)


def assert_logprobs(tok_lp, top_id, top_lp, oracle, n_top, what: str = "") -> float:
    """One record row ``tok_lp`` [B], ``top_id`` / ``top_lp`` [B, 20] against :func:`token_logprobs`'s
    result: ids exactly, values within :func:`logprob_tol`, -inf / NaN in place, over the rows
    with ``n_top >= 0``. Returns the worst error / tolerance."""
    e_tok, e_id, e_lp, lse, l_tok, l_top = oracle
    rows = torch.as_tensor(n_top).cpu() >= 0
    if not bool(rows.any()):
        return 0.0
    got_id = top_id.detach().cpu().long()[rows]
    bad = got_id != e_id[rows]
    assert not bool(bad.any()), (f"{what}: top ids differ at {bad.nonzero()[0].tolist()} (of the asking rows): "
                                 f"got {got_id[bad][0].item()}, oracle {e_id[rows][bad][0].item()}")
    r1 = assert_within(tok_lp.detach().cpu()[rows], e_tok[rows], logprob_tol(e_tok[rows], l_tok[rows], lse[rows]),
                       what + " tok_lp", dtype=torch.float32)
    r2 = assert_within(top_lp.detach().cpu()[rows], e_lp[rows],
                       logprob_tol(e_lp[rows], l_top[rows], lse[rows][:, None]), what + " top_lp",
                       dtype=torch.float32)
    return max(r1, r2)


# ---- attention (csrc/attn_core.h, attention_decode.hip, attention_prefill32.hip, attention_prefill.hip) ----
# Tolerance of one output element: attn_tol(e, A, p_exact) = bf16_ulp(e) + ((0 if p_exact else 2^-9)
# + ATTN_SLACK) * A, with A = sum_j w_j |v_j[d]| the softmax-weighted mean of |V| in that dimension
# (derivation: the module docstring). ATTN_P_ROUND is the unit round-off of bf16, 2^-8: the relative
# error of rounding one p to nearest. ATTN_SLACK is measured, not derived: the worst |o32 - e| / A of
# the fp32 CPU REFERENCE (ops/reference.py, its output before the bf16 cast) over every case of the
# lists below (ATTN_REF_WORST; tests/test_attention_oracle_cpu.py recomputes and prints it), times 4
# for the device's exp2, its tile order and its merges, rounded up to a power of two. The worst
# cases are the steep ramps: at 8 log2 units per key the scores reach 2048, where one fp32 rounding
# of a score moves the runner-up's weight by 1e-4 of itself, and A is small where the dominant key's
# value is. It is not tuned against the kernels.
ATTN_P_ROUND = 2.0 ** -8
ATTN_REF_WORST = 1.12e-4         # measured (tests/test_attention_oracle_cpu.py::test_reference_worst_is_recorded
#                                  prints it: 1.115e-4 at the key-split prefill case (32, 8, 128), ramp_r8)
ATTN_SLACK = 2.0 ** -11          # 4 * 1.12e-4 = 4.48e-4 <= 2^-11 = 4.88e-4
ATTN_BS = 32
ATTN_POISON_V = 96.0

ATTN_KINDS = ("random", "peaky", "census", "ramp_r025", "ramp_r8", "ramp_f025", "ramp_f8", "ramp_r006", "onehot")
ATTN_RAMP = {"ramp_r025": (0.25, False), "ramp_r8": (8.0, False), "ramp_f025": (0.25, True), "ramp_f8": (8.0, True),
             "ramp_r006": (0.0625, False)}
ATTN_RAMP_KEYS = 256

ATTN_DECODE_CFGS = ((32, 8, 128), (8, 1, 128), (16, 1, 128), (28, 4, 128), (12, 12, 64), (14, 2, 64))
ATTN_DECODE_SPLITS = (1, 3, 8, 64)
ATTN_DECODE_LENS = (1, 31, 32, 33, 64, 65, 257, 1500)
ATTN_REFILL_CFGS = ((8, 1, 128), (32, 8, 128))
ATTN_REFILL_LENS = (16417, 40)
ATTN_REFILL_SPLITS = (1, 2)
ATTN_REFILL_KINDS = ("census", "onehot")
ATTN_GROUP_CFGS = ((32, 8, 128), (8, 1, 128), (28, 4, 128), (12, 12, 64))
ATTN_GROUP_SPLITS = (1, 3, 8, 10, 64)
# (group label or None, shared blocks, context lengths): a 3-member table with 5 shared blocks and
# tails of 1 / 33 / 300 keys (at G = 8: wider than 16 columns, cut into sub-groups), a lone row
# between two groups, 4 members over 3 shared blocks (at G = 4 a full 16-column group) one of which
# has no private tile, a group with 0 shared blocks, and 2 members over 60 shared blocks
ATTN_GROUP_LAYOUT = (("A", 5, (161, 193, 460)), (None, 0, (77,)), ("B", 3, (96, 101, 160, 136)),
                     ("C", 0, (40, 70)), ("D", 60, (1927, 2420)))
ATTN_PREFILL_CFGS = ((32, 8, 128), (28, 4, 128), (12, 4, 128), (16, 1, 128), (12, 12, 64), (14, 2, 64))
ATTN_PREFILL_SPECS = ((0, 1), (0, 33), (0, 64), (0, 65), (31, 33), (63, 2), (64, 64), (127, 70), (128, 1), (500, 17),
                      (0, 257))
ATTN_SPLIT_CFGS = ((4, 1, 128), (8, 2, 128), (28, 4, 128), (32, 8, 128))
ATTN_SPLIT_SPECS = ((2345, 129), (0, 257), (31, 1), (9000, 300))
ATTN_SPLIT_MIN_CHUNK = (1, 3)


class AttnCase:
    """One attention test input, CPU tensors: ``q`` [rows, Hq, D] bf16, the paged ``k_cache`` /
    ``v_cache``, ``block_tables`` [S, max_blocks] int32 (padding entries: ``poison_block``),
    ``specs`` = (start, new) per sequence, ``ctx_lens`` / ``cu_q`` / ``start_pos`` int32,
    ``group_of`` / ``shared`` per sequence (:func:`ops.decode_groups` operands), ``scale``,
    ``p_exact``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _attn_rows64(qs, k, v, pos, scale):
    """fp64 attention of rows ``qs`` [R, Hq, D] over keys ``k`` / ``v`` [n, Hkv, D]; row i sees the
    keys 0..pos[i]. -> (e, A) [R, Hq, D]."""
    R, Hq, D = qs.shape
    n, Hkv, _ = k.shape
    G = Hq // Hkv
    e = torch.empty(R, Hq, D, dtype=torch.float64)
    A = torch.empty_like(e)
    hidden = torch.arange(n)[None, :] > pos[:, None]                      # [R, n]
    for h in range(Hkv):
        qh = qs[:, h * G:(h + 1) * G].double()
        s = torch.matmul(qh, k[:, h].double().t()) * scale                 # [R, G, n]
        s.masked_fill_(hidden[:, None, :], float("-inf"))
        w = torch.softmax(s, dim=-1)
        vh = v[:, h].double()
        e[:, h * G:(h + 1) * G] = torch.matmul(w, vh)
        A[:, h * G:(h + 1) * G] = torch.matmul(w, vh.abs())
    return e, A


def _attn_gather(k_cache, v_cache, bt_row, n):
    """Keys / values 0..n-1 of one block-table row, as ops/reference.py gathers them: K through
    ``k_rows`` (chunk-major blocks), V from the transposed ``[block, head, D, 32]`` layout."""
    from .reference import k_rows
    bs = k_cache.shape[2]
    nblk = (n + bs - 1) // bs
    blocks = bt_row[:nblk].long()
    k = k_rows(k_cache, blocks)[:n]
    v = v_cache[blocks].permute(0, 3, 1, 2).reshape(nblk * bs, v_cache.shape[1], -1)[:n]
    return k, v


def paged_attention_decode64(q, k_cache, v_cache, block_tables, ctx_lens, scale):
    """fp64 twin of ops.paged_attention_decode: ``(e, A)`` [B, Hq, D], unrounded."""
    B = q.shape[0]
    e = torch.empty(q.shape, dtype=torch.float64)
    A = torch.empty_like(e)
    for b in range(B):
        n = int(ctx_lens[b])
        k, v = _attn_gather(k_cache, v_cache, block_tables[b], n)
        e[b:b + 1], A[b:b + 1] = _attn_rows64(q[b:b + 1], k, v, torch.tensor([n - 1]), scale)
    return e, A


def prefill_attention64(q, k_cache, v_cache, block_tables, cu_q, start_pos, scale):
    """fp64 twin of ops.prefill_attention (row i of sequence s sees keys 0..start_pos[s] + i):
    ``(e, A)`` [T, Hq, D], unrounded."""
    e = torch.zeros(q.shape, dtype=torch.float64)
    A = torch.zeros_like(e)
    for s in range(cu_q.shape[0] - 1):
        a, b = int(cu_q[s]), int(cu_q[s + 1])
        if b == a:
            continue
        st = int(start_pos[s])
        k, v = _attn_gather(k_cache, v_cache, block_tables[s], st + b - a)
        e[a:b], A[a:b] = _attn_rows64(q[a:b], k, v, torch.arange(st, st + b - a), scale)
    return e, A


def attn_tol(e, A, p_exact: bool = False):
    return bf16_ulp(e) + ((0.0 if p_exact else ATTN_P_ROUND) + ATTN_SLACK) * A.double()


def error_ratio(got, e, tol) -> float:
    """Worst ``|got - e| / tol`` (no assertion; 0 / 0 counts as 0): how far a deliberately wrong
    result lies outside a tolerance."""
    d = (got.detach().cpu().double().reshape(-1) - e.double().reshape(-1)).abs()
    t = tol.double().reshape(-1)
    r = torch.where(d > 0, d / t, torch.zeros_like(d))
    r = torch.where(torch.isfinite(d), r, torch.full_like(d, float("inf")))     # NaN / inf: outside
    return float(r.max()) if r.numel() else 0.0


def attn_marks(L: int, lo: int = 0) -> List[int]:
    """The boundary keys of a row of ``L`` keys (wrapped into the row when it is short), those at
    or past ``lo``: 0, 7, 8, 31, 32, L-33, L-32, L-2, L-1, L/2, and the last key of tile 510 and the
    first and last keys of tiles 511 and 512 (the plan row's limit) where the row has them."""
    cand = [0, 7, 8, 31, 32, L - 33, L - 32, L - 2, L - 1, L // 2]
    cand += [j for j in (511 * 32 - 1, 511 * 32, 512 * 32 - 1, 512 * 32, 513 * 32 - 1) if j < L]
    out: List[int] = []
    for c in cand:
        c %= L
        if c >= lo and c not in out:
            out.append(c)
    return out


def _attn_seq(kind, qs, st, new, hkv, d, scale, u, g, lo):
    """Logical K, V [L, hkv, d] (float, bf16-exact) of one sequence for rows ``qs`` [new, hq, d]
    (float) at positions st..st+new-1; ``lo``: first key this sequence owns (shared members)."""
    L = st + new
    hq = qs.shape[1]
    G = hq // hkv
    K = torch.randn(L, hkv, d, generator=g)
    V = torch.randn(L, hkv, d, generator=g)
    if kind == "census":
        K.zero_()
        V.zero_()
        marks = attn_marks(L)
        for i in range(d // 2):
            V[marks[i % len(marks)], :, i] = 1.0
        j = torch.arange(L)
        V[j, :, d // 2 + (j // ATTN_BS) % (d // 2)] = 1.0
    elif kind in ATTN_RAMP:
        gap, falling = ATTN_RAMP[kind]
        # scores rise (fall) by about ``gap`` log2 units per key: q . u = 8 d, c a power of two
        c = 2.0 ** round(math.log2(gap / (8.0 * d * scale * math.log2(math.e))))
        n = min(L, ATTN_RAMP_KEYS)
        r = torch.zeros(L)
        if falling:
            r[:n] = torch.arange(n, 0, -1, dtype=torch.float32)
        else:
            r[L - n:] = torch.arange(1, n + 1, dtype=torch.float32)
        K = (r * c)[:, None, None] * u[None]
    elif kind == "onehot":
        K *= 0.05
        marks = attn_marks(L, lo)
        qm = qs.reshape(new, hkv, G, d).mean(2)                             # [new, hkv, d]
        if new == 1:        # decode: one key per (row, kv head)
            for h in range(hkv):
                if marks:
                    K[marks[(st + h) % len(marks)], h] = 4.0 * qm[0, h]
        else:               # prefill: the boundary keys, each aligned with the first row that sees it
            for i, mk in enumerate(marks):
                K[mk] = 4.0 * qm[mk - st if mk >= st else i % new]
    return K.to(torch.bfloat16).float(), V.to(torch.bfloat16).float()


def attn_case(kind: str, hq: int, hkv: int, d: int, specs, layout=None, seed: int = 0) -> AttnCase:
    """One attention input of ``kind`` (ATTN_KINDS) for sequences ``specs`` = (start, new) (decode:
    (ctx - 1, 1)), ``layout`` = (label, shared blocks) per sequence for shared-prefix groups.

    random: N(0,1) q, K, V. peaky: q x 6 (largest weight 0.7..0.99). census: K = 0, V = 0/1 markers
    (dims < D/2 one boundary key each, :func:`attn_marks`; dims >= D/2 the tile classes
    ``(j // 32) % (D/2)``): outputs are counts / L, p_exact. ramp_*: K = r_j c u over 256 positions
    (rising: the last, falling: the first), 0 elsewhere, r_j integers and c a power of two so K is
    exact; q = 8 u + 0.25 noise; nominal gap 0.0625 / 0.25 / 8 log2 units per key. onehot: one key
    per (row, kv head) at a boundary position aligned with the group's mean query x 4, other K x 0.05.

    Poison, every kind: K = 8 x (mean query of the rows that could reach the slot) per kv head,
    V = 96, in every slot of a row's last block at or past its end, in every block no row references
    and in one dedicated block every block-table padding entry points to. All finite."""
    from .reference import write_k
    bs = ATTN_BS
    S = len(specs)
    g = _gen(5000 + 97 * ATTN_KINDS.index(kind) + 13 * hq + 7 * hkv + d + 31 * sum(a + 3 * b for a, b in specs)
             + 1009 * seed)
    G = hq // hkv
    scale = 1.0 / math.sqrt(d)
    u = torch.where(torch.rand(hkv, d, generator=g) < 0.5, -1.0, 1.0)
    layout = [(None, 0)] * S if layout is None else list(layout)
    qs_all, kv_all, first = [], [], {}
    for s, (st, new) in enumerate(specs):
        label, sh = layout[s]
        member0 = first.setdefault(label, s) if label is not None and sh > 0 else s
        qs = torch.randn(new, hq, d, generator=g)
        if kind == "peaky":
            qs = qs * 6.0
        elif kind in ATTN_RAMP:
            qs = 8.0 * u.repeat_interleave(G, 0)[None] + 0.25 * qs
        qs = qs.to(torch.bfloat16).float()
        own = sh * bs if member0 != s else 0
        K, V = _attn_seq(kind, qs, st, new, hkv, d, scale, u, g, own)
        if own:
            K[:own], V[:own] = kv_all[member0][0][:own], kv_all[member0][1][:own]
        qs_all.append(qs)
        kv_all.append((K, V))
    # physical placement: shared blocks once per group, then each row's own; + the dedicated poison
    # block + 3 blocks nobody references, ids shuffled
    nblk = [(st + new + bs - 1) // bs for st, new in specs]
    need = sum(nblk[s] - (layout[s][1] if first.get(layout[s][0], s) != s else 0) for s in range(S))
    nb = need + 4
    perm = torch.randperm(nb, generator=g).tolist()
    poison_block = perm.pop()
    maxb = max(nblk) + 2
    bt = torch.full((S, maxb), poison_block, dtype=torch.int32)
    for s in range(S):
        label, sh = layout[s]
        m0 = first.get(label, s) if label is not None and sh > 0 else s
        keep = sh if m0 != s else 0
        bt[s, :keep] = bt[m0, :keep]
        bt[s, keep:nblk[s]] = torch.tensor([perm.pop() for _ in range(nblk[s] - keep)], dtype=torch.int32)
    q = torch.cat(qs_all).to(torch.bfloat16)
    qmean = lambda t: t.reshape(-1, hkv, G, d).mean((0, 2))                   # noqa: E731  [hkv, d]
    k_cache = torch.empty(nb, hkv, bs, d, dtype=torch.bfloat16)
    v_cache = torch.full((nb, hkv, d, bs), ATTN_POISON_V, dtype=torch.bfloat16)
    allb, off = torch.arange(nb).repeat_interleave(bs), torch.arange(bs).repeat(nb)
    write_k(k_cache, allb, off, (8.0 * qmean(q.float()))[None].expand(nb * bs, hkv, d))
    for s, (st, new) in enumerate(specs):
        L = st + new
        pos = torch.arange(nblk[s] * bs)
        blk = bt[s, pos // bs].long()
        K = torch.cat([kv_all[s][0], (8.0 * qmean(qs_all[s]))[None].expand(nblk[s] * bs - L, hkv, d)])
        V = torch.cat([kv_all[s][1], torch.full((nblk[s] * bs - L, hkv, d), ATTN_POISON_V)])
        write_k(k_cache, blk, pos % bs, K)
        v_cache[blk, :, :, pos % bs] = V.to(torch.bfloat16)
    cu = [0]
    for _, new in specs:
        cu.append(cu[-1] + new)
    return AttnCase(kind=kind, hq=hq, hkv=hkv, d=d, specs=tuple(specs), q=q, k_cache=k_cache, v_cache=v_cache,
                    block_tables=bt, poison_block=poison_block, scale=scale, p_exact=kind == "census",
                    ctx_lens=torch.tensor([a + b for a, b in specs], dtype=torch.int32),
                    cu_q=torch.tensor(cu, dtype=torch.int32),
                    start_pos=torch.tensor([a for a, _ in specs], dtype=torch.int32),
                    group_of=[lb for lb, _ in layout], shared=[sh for _, sh in layout])


def attn_decode_case(kind, hq, hkv, d, lens=ATTN_DECODE_LENS) -> AttnCase:
    return attn_case(kind, hq, hkv, d, [(l - 1, 1) for l in lens])


def attn_group_case(kind, hq, hkv, d) -> AttnCase:
    specs, layout = [], []
    for label, sh, lens in ATTN_GROUP_LAYOUT:
        for l in lens:
            specs.append((l - 1, 1))
            layout.append((label, sh))
    return attn_case(kind, hq, hkv, d, specs, layout)


def attn_table3_case(kind, hq, hkv, d) -> AttnCase:
    """The 3-member table of ATTN_GROUP_LAYOUT alone."""
    label, sh, lens = ATTN_GROUP_LAYOUT[0]
    return attn_case(kind, hq, hkv, d, [(l - 1, 1) for l in lens], [(label, sh)] * len(lens))


def attn_case_fp8(case: AttnCase, k_scale: float = 1.0, v_scale: float = 1.0) -> AttnCase:
    """The fp8-KV twin of ``case`` (kv_dtype "fp8", ops/reference.py ``kv_fp8_code``): the same q,
    block tables and lengths; ``k_cache`` / ``v_cache`` hold the e4m3fn codes (uint8) of every slot of
    the bf16 caches, poison included, under ``k_scale`` / ``v_scale`` in the fp8 block byte order;
    ``k_deq`` / ``v_deq`` hold ``e4m3(code) * scale`` in fp64 in the bf16 caches' layout, which is
    what :func:`attn_oracle` of the twin computes from. The convert is exact and the two scale folds
    of the kernels (k_scale into the softmax scale, v_scale into the final 1/l) are fp32 roundings
    far inside ATTN_SLACK, so the twin's tolerance is ``attn_tol`` of its own oracle, unchanged.
    Every code is finite: inputs are finite and the encode saturates at +-448 (V poison 96 / v_scale
    and the K poison round to finite codes)."""
    from .reference import k_rows, kv_fp8_code, kv_fp8_inv, kv_fp8_value, write_k, write_k_fp8, write_v_fp8
    nb, hkv, bs, d = case.k_cache.shape
    blocks = torch.arange(nb)
    allb, off = blocks.repeat_interleave(bs), torch.arange(bs).repeat(nb)
    K = k_rows(case.k_cache, blocks).float()                                     # [nb * bs, hkv, d]
    V = case.v_cache[blocks].permute(0, 3, 1, 2).reshape(nb * bs, hkv, d).float()
    kc, vc = kv_fp8_code(K, kv_fp8_inv(k_scale)), kv_fp8_code(V, kv_fp8_inv(v_scale))
    # A NONZERO value whose code would be +-0 takes the smallest code of its sign (+-2^-9) instead; the
    # census kinds' exact zeros stay zero. Reason: e4m3 keeps 4 significant bits of K, which turns the
    # steepest ramp (8 log2 units per key) into plateaus of 16 equal keys 128 log2 units apart. Where a
    # plateau's only visible key had a zero V code, the exact output would be 2^-128 of the row's
    # largest weight: below the fp32 normal range relative to it, which neither attn_tol's derivation
    # (fp32 arithmetic without underflow) nor the kernels' exp2 (results below 2^-126 of the row
    # maximum are dropped, csrc/common.h fast_exp2) covers. bf16 inputs never have this structure
    # (their ramps are exact and a random bf16 V is never exactly 0); the twin must not add it.
    lost = (V != 0) & ((vc & 0x7F) == 0)
    vc = torch.where(lost, (vc & 0x80) | 1, vc)
    k8 = torch.zeros(nb, hkv, bs, d, dtype=torch.uint8)
    v8 = torch.zeros(nb, hkv, d, bs, dtype=torch.uint8)
    write_k_fp8(k8, allb, off, kc)
    write_v_fp8(v8, allb, off, vc)
    kd = torch.empty(nb, hkv, bs, d, dtype=torch.float64)
    vd = torch.empty(nb, hkv, d, bs, dtype=torch.float64)
    write_k(kd, allb, off, kv_fp8_value(kc).double() * float(k_scale))
    vd[allb, :, :, off] = kv_fp8_value(vc).double() * float(v_scale)
    assert bool(torch.isfinite(kd).all()) and bool(torch.isfinite(vd).all())
    twin = AttnCase(**case.__dict__)
    twin.k_cache, twin.v_cache, twin.k_deq, twin.v_deq = k8, v8, kd, vd
    twin.k_scale, twin.v_scale = float(k_scale), float(v_scale)
    twin.v_lifted = int(lost.sum())      # V codes that are not kv_fp8_code's own (tests bound the count)
    return twin


def attn_oracle(case: AttnCase, prefill: bool = False):
    """-> (e, A, tol) of ``case``; an fp8 twin (:func:`attn_case_fp8`) is judged on its dequantised values."""
    kc, vc = (case.k_deq, case.v_deq) if hasattr(case, "k_deq") else (case.k_cache, case.v_cache)
    if prefill:
        e, A = prefill_attention64(case.q, kc, vc, case.block_tables, case.cu_q, case.start_pos, case.scale)
    else:
        e, A = paged_attention_decode64(case.q, kc, vc, case.block_tables, case.ctx_lens, case.scale)
    return e, A, attn_tol(e, A, case.p_exact)


def attn_prefill_rows(G: int, d: int) -> int:
    """Query rows of one prefill work tile (csrc/attention_prefill.hip prefill_rows_per_tile; the GPU
    test holds the two together): the 32x32 kernel for D = 128 and G <= 8, else the 16x16 one."""
    if d == 128 and G <= 8:
        return 32 * 8 // (1 if G == 1 else 2 if G == 2 else 4 if G <= 4 else 8)
    return 16 if G >= 4 else 16 * (4 // G)
