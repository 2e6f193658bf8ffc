"""The fp64 oracle (ops/oracle64.py) and its tolerances are sound without a GPU: fp32 emulations
of the kernels' arithmetic, written here in PyTorch, pass ``assert_within`` on the very inputs
tests/test_elementwise_gpu.py feeds the HIP kernels. The emulations follow the kernels' formulas,
not their reduction order."""
import pytest
import torch

from theroundtaible_amd.ops import oracle64 as o64
from theroundtaible_amd.ops import reference as ref

BF = torch.bfloat16


# ---- fp32 emulations of csrc/norm.hip, activation.hip, rope_cache.hip ------------------------

def emu_rms(x, w, eps):
    xf = x.float()
    inv = torch.rsqrt((xf * xf).sum(-1, keepdim=True) / x.shape[-1] + eps)
    return (xf * inv * w.float()).to(BF)


def emu_ln(x, w, b, eps, two_pass=True):
    xf = x.float()
    H = x.shape[-1]
    s = xf.sum(-1, keepdim=True)
    mean = s / H
    if two_pass:
        # the division's remainder fmaf(-mean, H, s), exact in the kernel: fp64 here, rounded once
        mean_lo = ((s.double() - mean.double() * H) / H).float()
        d = (xf - mean) - mean_lo
        var = (d * d).sum(-1, keepdim=True) / H
    else:                                       # E[x^2] - mean^2: what norm.hip did before
        d = xf - mean
        var = ((xf * xf).sum(-1, keepdim=True) / H - mean * mean).clamp_min(0.0)
    inv = torch.rsqrt(var + eps)
    return (d * inv * w.float() + b.float()).to(BF)


def emu_silu_mul(x):
    i = x.shape[-1] // 2
    g, u = x[..., :i].float(), x[..., i:].float()
    return (g / (1.0 + torch.exp(-g)) * u).to(BF)


def emu_gelu(x):
    xf = x.float()
    k0, k1 = torch.tensor(o64.GELU_K0, dtype=torch.float32), torch.tensor(o64.GELU_K1, dtype=torch.float32)
    return (0.5 * xf * (1.0 + torch.tanh(k0 * (xf + k1 * xf * xf * xf)))).to(BF)


def emu_rope(x, cs):
    h = x.shape[-1] // 2
    c, s = cs[:, None, :h], cs[:, None, h:]
    x1, x2 = x[..., :h].float(), x[..., h:].float()
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(BF)


# ---- the oracle itself -----------------------------------------------------------------------

def test_bf16_ulp():
    t = torch.tensor([1.0, 1.99, 2.0, -3.0, 0.0, 2.0 ** -126, 2.0 ** -130, 3e38, 0.75], dtype=torch.float64)
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133, 2.0 ** -133,
                         2.0 ** 120, 2.0 ** -8], dtype=torch.float64)
    assert torch.equal(o64.bf16_ulp(t), want)
    # it is the distance to the next bf16 for every finite positive pattern below the largest
    tab = o64.finite_bf16_table()
    pos = tab[(tab > 0) & (tab.view(torch.int16) < 0x7F7F)]
    nxt = (pos.view(torch.int16) + 1).view(BF)
    assert torch.equal(o64.bf16_ulp(pos), nxt.double() - pos.double())


def test_finite_table():
    tab = o64.finite_bf16_table()
    assert tab.numel() == 65280 and bool(torch.isfinite(tab).all())
    assert tab.view(torch.int16).unique().numel() == 65280


def test_assert_within_catches_one_ulp_and_nonfinite():
    e = torch.tensor([1.0, -2.5, 100.0, 1e-3], dtype=torch.float64)
    tol = o64.bf16_ulp(e)
    good = e.to(BF)
    assert o64.assert_within(good, e, tol) <= 0.5          # correct rounding: half an ulp
    two_ulp = (good.view(torch.int16) + 2).view(BF)
    with pytest.raises(AssertionError):
        o64.assert_within(two_ulp, e, tol)
    for bad in (float("nan"), float("inf"), float("-inf")):
        g = good.clone()
        g[2] = bad
        with pytest.raises(AssertionError):
            o64.assert_within(g, e, tol)
    # an oracle value that rounds to inf demands inf, with the sign
    big = torch.tensor([3.4e38, -3.4e38], dtype=torch.float64)
    o64.assert_within(torch.tensor([float("inf"), float("-inf")], dtype=BF), big, o64.bf16_ulp(big))
    with pytest.raises(AssertionError):
        o64.assert_within(torch.tensor([float("inf"), float("inf")], dtype=BF), big, o64.bf16_ulp(big))


def test_oracle_agrees_with_fp32_reference():
    """The fp64 oracle and ops/reference.py describe the same operations."""
    g = torch.Generator().manual_seed(3)
    x, r = (torch.randn(4, 64, generator=g).to(BF) for _ in range(2))
    w, b = o64.norm_params(64)
    for (e, mag), want in (
            (o64.rms_norm(x, w, 1e-5), ref.rms_norm(x, w, 1e-5)),
            (o64.layer_norm(x, w, b, 1e-5), ref.layer_norm(x, w, b, 1e-5)),
            (o64.fused_add_rms_norm(x, r, w, 1e-5)[:2], ref.fused_add_rms_norm(x, r, w, 1e-5)[0]),
            (o64.fused_add_layer_norm(x, r, w, b, 1e-5)[:2], ref.fused_add_layer_norm(x, r, w, b, 1e-5)[0]),
            (o64.silu_and_mul(x), ref.silu_and_mul(x)),
            (o64.gelu_tanh(x), ref.gelu_tanh(x))):
        o64.assert_within(want, e, o64.bf16_ulp(e) + 2.0 ** -14 * mag)
    assert torch.equal(o64.fused_add_rms_norm(x, r, w, 1e-5)[2], ref.fused_add_rms_norm(x, r, w, 1e-5)[1])
    cs = ref.rope_cos_sin(16, 64, 10000.0)[torch.tensor([0, 5, 9, 15])]
    e, mag = o64.rope(x.reshape(4, 1, 64), cs)
    o64.assert_within(ref._rotate(x.reshape(4, 1, 64).float(), cs).to(BF), e, o64.rope_tol(e, mag))


# ---- emulations on the GPU test's inputs -----------------------------------------------------

def _norm_shapes(H):
    return [(rows, H) for rows in o64.NORM_ROWS] + [(2, 3, H)]


@pytest.mark.parametrize("H", o64.NORM_H)
def test_rms_emulation_within_tolerance(H):
    w, _ = o64.norm_params(H)
    for shape in _norm_shapes(H):
        for name, x, _, eps in o64.norm_cases(shape, ln=False, add=False):
            e, mag = o64.rms_norm(x, w, eps)
            o64.assert_within(emu_rms(x, w, eps), e, o64.norm_tol(e, mag), f"rms {shape} {name}")
        for name, x, r, eps in o64.norm_cases(shape, ln=False, add=True):
            e, mag, res = o64.fused_add_rms_norm(x, r, w, eps)
            o64.assert_within(emu_rms(res, w, eps), e, o64.norm_tol(e, mag), f"add rms {shape} {name}")


@pytest.mark.parametrize("H", o64.NORM_H)
def test_two_pass_layernorm_emulation_within_tolerance(H):
    w, b = o64.norm_params(H)
    for shape in _norm_shapes(H):
        for name, x, _, eps in o64.norm_cases(shape, ln=True, add=False):
            e, mag = o64.layer_norm(x, w, b, eps)
            o64.assert_within(emu_ln(x, w, b, eps), e, o64.norm_tol(e, mag), f"ln {shape} {name}")
            if name == "const3":
                o64.assert_within(emu_ln(x, w, b, eps), b.double().expand_as(e), o64.norm_tol(e, mag))
        for name, x, r, eps in o64.norm_cases(shape, ln=True, add=True):
            e, mag, res = o64.fused_add_layer_norm(x, r, w, b, eps)
            o64.assert_within(emu_ln(res, w, b, eps), e, o64.norm_tol(e, mag), f"add ln {shape} {name}")


@pytest.mark.parametrize("H", [768, 8192])
def test_one_pass_layernorm_variance_fails_offset_rows(H):
    """Why norm.hip takes a second pass for the LayerNorm variance: var = E[x^2] - mean^2 in fp32
    loses the variance of a row whose mean is large against its spread (3000 +- 16: x^2 ~ 9e6
    carries an fp32 error of ~1 against a variance of 256), and the outputs leave the tolerance.
    sum((x - mean)^2) on the same rows stays inside it."""
    w, b = o64.norm_params(H)
    x = (3000.0 + 16.0 * torch.randn(64, H, generator=torch.Generator().manual_seed(H))).to(BF)
    e, mag = o64.layer_norm(x, w, b, 1e-5)
    tol = o64.norm_tol(e, mag)
    o64.assert_within(emu_ln(x, w, b, 1e-5, two_pass=True), e, tol, "two-pass")
    with pytest.raises(AssertionError):
        o64.assert_within(emu_ln(x, w, b, 1e-5, two_pass=False), e, tol, "one-pass")


def test_silu_emulation_within_tolerance():
    for name, x in list(o64.silu_inputs().items()) + [("stride", o64.silu_stride_input())]:
        e, mag = o64.silu_and_mul(x)
        o64.assert_within(emu_silu_mul(x), e, o64.silu_tol(e, mag), f"silu {name}")


def test_gelu_emulation_within_tolerance():
    for name, x in list(o64.gelu_inputs().items()) + [("stride", o64.gelu_stride_input())]:
        e, mag = o64.gelu_tanh(x)
        o64.assert_within(emu_gelu(x), e, o64.gelu_tol(e, mag), f"gelu {name}")
    # a pure-ulp tolerance would be wrong: 1 + tanh cancels for x in [-7, -4]
    x = o64.finite_bf16_table()
    e, _ = o64.gelu_tanh(x)
    with pytest.raises(AssertionError):
        o64.assert_within(emu_gelu(x), e, o64.bf16_ulp(e) + o64.FLOOR)


@pytest.mark.parametrize("hq,hkv,D", o64.ROPE_SHAPES)
@pytest.mark.parametrize("T", o64.ROPE_T)
def test_rope_emulation_within_tolerance(hq, hkv, D, T):
    cos_sin = ref.rope_cos_sin(o64.ROPE_MAX_POS, D, o64.ROPE_THETA)
    for first in (0, o64.ROPE_MAX_POS - 1):
        qkv, pos, slots, kc, vc = o64.rope_case(hq, hkv, D, T, first_pos=first)
        assert slots.unique().numel() == T and int(pos[0]) == first
        assert T == 1 or {0, o64.ROPE_MAX_POS - 1} <= set(pos.tolist()) or first != 0
        x = qkv[:, :(hq + hkv) * D].reshape(T, hq + hkv, D)
        e, mag = o64.rope(x, cos_sin[pos])
        o64.assert_within(emu_rope(x, cos_sin[pos]), e, o64.rope_tol(e, mag), "rope")
        if first == 0:                          # cos = 1, sin = 0: the input bits
            assert torch.equal(e[0], x[0].double())
    e, mag = o64.rope(x, None)
    assert torch.equal(e, x.double())
