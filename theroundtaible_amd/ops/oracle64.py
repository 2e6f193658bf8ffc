"""fp64 oracle of the elementwise kernels (csrc/norm.hip, activation.hip, rope_cache.hip).

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

The input builders of the CPU emulation test and the GPU test live here too, so both see the
same bits.
"""
from __future__ import annotations

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


def assert_within(got: torch.Tensor, e: torch.Tensor, tol: torch.Tensor, what: str = "") -> float:
    """``|got - e| <= tol`` wherever ``e`` rounds to a finite bf16; NaN, +inf and -inf of ``got``
    sit exactly where ``e`` rounded to bf16 has them. Returns the worst error / tolerance."""
    assert got.dtype == torch.bfloat16, f"{what}: output is {got.dtype}, not bfloat16"
    g = got.detach().cpu().double().reshape(-1)
    e = e.double().reshape(-1)
    tol = tol.double().reshape(-1)
    assert g.shape == e.shape == tol.shape, f"{what}: shapes {tuple(g.shape)} {tuple(e.shape)} {tuple(tol.shape)}"
    if g.numel() == 0:
        return 0.0
    eb = e.float().to(torch.bfloat16).double()
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
