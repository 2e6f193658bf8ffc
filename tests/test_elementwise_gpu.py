"""csrc/norm.hip, activation.hip, rope_cache.hip and their checks in csrc/bindings.cpp against the
fp64 oracle (ops/oracle64.py) at one-bf16-ulp tolerances: the multi-chunk norm path, partly filled
waves, value regimes where eps / outliers / a row offset matter, every finite bf16 input of the
activations, the second trip of their grid-stride loops, strided qkv rows, and the cache elements
rope_and_cache must not touch. Each case prints its worst error / tolerance (``pytest -s``).

Measured on an MI355X: every kernel's worst ratio is 0.50 (one correct bf16 rounding of the fp64
value). With the former one-pass LayerNorm variance (E[x^2] - mean^2) the offset rows missed by up
to 17x (-20000 +- 100 at H = 896; 3000 +- 16: 16.8x at H = 520 and 16384)."""
import pytest
import torch

from theroundtaible_amd import ops
from theroundtaible_amd.ops import oracle64 as o64
from theroundtaible_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def report(kernel, case, ratio):
    print(f"RATIO {kernel} {case} {ratio:.3f}")


# ---- norms -------------------------------------------------------------------------------------

NORM_SHAPES = [(rows, H) for H in o64.NORM_H for rows in o64.NORM_ROWS] + [(2, 3, 896), (2, 3, 8200)]


def run_norm(ln, add, x, r, w, b, eps):
    """-> (out, updated residual or None) of the HIP kernel."""
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    if add:
        rd = r.to(DEV)
        out, res = (ops.fused_add_layer_norm(xd, rd, wd, bd, eps) if ln else ops.fused_add_rms_norm(xd, rd, wd, eps))
        assert res.data_ptr() == rd.data_ptr()
        assert torch.equal(bits(xd), bits(x)), "the kernel wrote its input"
        return out, res
    return (ops.layer_norm(xd, wd, bd, eps) if ln else ops.rms_norm(xd, wd, eps)), None


def oracle_norm(ln, add, x, r, w, b, eps):
    res = o64.add_residual(x, r) if add else None
    e, mag = o64.layer_norm(res if add else x, w, b, eps) if ln else o64.rms_norm(res if add else x, w, eps)
    return e, mag, res


@pytest.mark.parametrize("shape", NORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("ln", [False, True], ids=["rms", "layer"])
@pytest.mark.parametrize("add", [False, True], ids=["plain", "fused_add"])
def test_norm(shape, ln, add):
    H = shape[-1]
    w, b = o64.norm_params(H)
    name = ("fused_add_" if add else "") + ("layer_norm" if ln else "rms_norm")
    for case, x, r, eps in o64.norm_cases(shape, ln, add):
        out, res = run_norm(ln, add, x, r, w, b, eps)
        assert out.shape == x.shape
        e, mag, want_res = oracle_norm(ln, add, x, r, w, b, eps)
        tol = o64.norm_tol(e, mag)
        what = f"{name} {shape} {case}"
        if add:
            assert torch.equal(bits(res), bits(want_res)), f"{what}: residual bits"
        report(name, f"{shape} {case}", o64.assert_within(out, e, tol, what))
        if ln and case == "const3":         # zero variance: the bias
            o64.assert_within(out, b.double().expand_as(e), tol, what + " (bias)")


@pytest.mark.parametrize("ln", [False, True], ids=["rms", "layer"])
@pytest.mark.parametrize("add", [False, True], ids=["plain", "fused_add"])
def test_norm_no_rows(ln, add):
    H = 896
    w, b = o64.norm_params(H)
    x = torch.empty(0, H, dtype=BF)
    out, res = run_norm(ln, add, x, x.clone(), w, b, 1e-5)
    assert out.shape == (0, H) and out.dtype == BF


@pytest.mark.parametrize("ln", [False, True], ids=["rms", "layer"])
@pytest.mark.parametrize("add", [False, True], ids=["plain", "fused_add"])
def test_norm_refusals(ln, add):
    """Rejected by the binding before any launch."""
    def call(x, H):
        w, b = o64.norm_params(H)
        run_norm(ln, add, x, x.clone(), w, b, 1e-5)

    for H in (100, 32776):                                  # not a multiple of 8; wider than a block holds
        with pytest.raises(RuntimeError, match="hidden size"):
            call(torch.zeros(2, H, dtype=BF), H)
    w, b = (t.to(DEV) for t in o64.norm_params(896))
    x = torch.zeros(4, 896, dtype=BF, device=DEV)
    nat = ops.native()

    def native_call(x, out, r):
        args = (out, x) + ((r,) if add else ()) + (w,) + ((b,) if ln else ()) + (1e-5,)
        getattr(nat, ("fused_add_" if add else "") + ("layer_norm" if ln else "rms_norm"))(*args)

    with pytest.raises(RuntimeError, match="contiguous"):   # row-strided input
        native_call(x[::2], torch.empty(2, 896, dtype=BF, device=DEV), torch.zeros(2, 896, dtype=BF, device=DEV))
    with pytest.raises(RuntimeError, match="bfloat16"):
        native_call(x.float(), torch.empty_like(x), torch.zeros_like(x))


# ---- activations -------------------------------------------------------------------------------

def check_silu(name, x):
    out = ops.silu_and_mul(x.to(DEV))
    assert out.shape == (*x.shape[:-1], x.shape[-1] // 2)
    e, mag = o64.silu_and_mul(x)
    report("silu_and_mul", name, o64.assert_within(out, e, o64.silu_tol(e, mag), f"silu_and_mul {name}"))


def check_gelu(name, x):
    out = ops.gelu_tanh(x.to(DEV))
    assert out.shape == x.shape
    e, mag = o64.gelu_tanh(x)
    report("gelu_tanh", name, o64.assert_within(out, e, o64.gelu_tol(e, mag), f"gelu_tanh {name}"))


@pytest.mark.parametrize("name", ["table_up1", "table_uprand", "rows1_I8", "rows3_I24"])
def test_silu_and_mul(name):
    check_silu(name, o64.silu_inputs()[name])


@pytest.mark.parametrize("name", ["table", "n8"])
def test_gelu_tanh(name):
    check_gelu(name, o64.gelu_inputs()[name])


def test_silu_and_mul_grid_stride_second_trip():
    x = o64.silu_stride_input()
    assert x.shape[0] * (x.shape[1] // 16) > 2048 * 256
    check_silu("grid_stride", x)


def test_gelu_tanh_grid_stride_second_trip():
    x = o64.gelu_stride_input()
    assert x.numel() // 8 > 2048 * 256
    check_gelu("grid_stride", x)


def test_activation_refusals():
    with pytest.raises(RuntimeError, match="silu_and_mul shape"):
        ops.silu_and_mul(torch.zeros(2, 24, dtype=BF, device=DEV))      # width % 16 != 0
    with pytest.raises(RuntimeError, match="gelu shape"):
        ops.gelu_tanh(torch.zeros(12, dtype=BF, device=DEV))            # numel % 8 != 0


# ---- rope_and_cache ----------------------------------------------------------------------------

_COS_SIN = {}


def cos_sin_table(D):
    if D not in _COS_SIN:
        _COS_SIN[D] = ref.rope_cos_sin(o64.ROPE_MAX_POS, D, o64.ROPE_THETA)
    return _COS_SIN[D]


@pytest.mark.parametrize("hq,hkv,D", o64.ROPE_SHAPES)
@pytest.mark.parametrize("T", o64.ROPE_T)
@pytest.mark.parametrize("rope", [True, False], ids=["rope", "norope"])
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "column_slice"])
def test_rope_and_cache(hq, hkv, D, T, rope, strided):
    table = cos_sin_table(D) if rope else None
    for first_pos in ((0, o64.ROPE_MAX_POS - 1) if T == 1 else (0,)):
        qkv, pos, slots, kc0, vc0 = o64.rope_case(hq, hkv, D, T, first_pos=first_pos)
        width = qkv.shape[1]
        if strided:     # rows of a wider buffer; the offset keeps the kernel's 8-byte loads aligned
            buf = torch.full((T, width + 24), float("nan"), dtype=BF, device=DEV)
            qkv_d = buf[:, 8:8 + width]
            qkv_d.copy_(qkv)
            assert not qkv_d.is_contiguous() or T == 1
        else:
            qkv_d = qkv.to(DEV)
        kc, vc = kc0.to(DEV), vc0.to(DEV)
        q = ops.rope_and_cache(qkv_d, pos.to(DEV), table.to(DEV) if rope else None, kc, vc, slots.to(DEV),
                               hq, hkv, D)
        assert q.shape == (T, hq, D)
        kc, vc = kc.cpu(), vc.cpu()

        x = qkv[:, :(hq + hkv) * D].reshape(T, hq + hkv, D)
        e, mag = o64.rope(x, table[pos] if rope else None)
        tol = o64.rope_tol(e, mag)
        what = f"rope_and_cache {(hq, hkv, D)} T={T} rope={rope} strided={strided} pos0={first_pos}"
        k_written = ref.k_rows(kc, torch.arange(o64.ROPE_BLOCKS))[slots]            # [T, hkv, D]
        report("rope_and_cache.q", what, o64.assert_within(q, e[:, :hq], tol[:, :hq], what + " q"))
        report("rope_and_cache.k", what, o64.assert_within(k_written, e[:, hq:], tol[:, hq:], what + " k"))
        if not rope:
            assert torch.equal(bits(q), bits(x[:, :hq])) and torch.equal(bits(k_written), bits(x[:, hq:]))
        if first_pos == 0:                      # cos = 1, sin = 0: the input bits
            assert torch.equal(bits(q[0]), bits(x[0, :hq])), what + ": q at position 0"
            assert torch.equal(bits(k_written[0]), bits(x[0, hq:])), what + ": k at position 0"

        blk, off = slots // o64.ROPE_BS, slots % o64.ROPE_BS
        v = qkv[:, (hq + hkv) * D:].reshape(T, hkv, D)
        assert torch.equal(bits(vc[blk, :, :, off]), bits(v)), what + ": v rows"
        # every element no slot addresses keeps its bits (masks built through the layouts' own views)
        k_mask, v_mask = torch.zeros(kc.shape, dtype=torch.bool), torch.zeros(vc.shape, dtype=torch.bool)
        ref.k_blocks(k_mask)[blk, :, :, off, :] = True
        v_mask[blk, :, :, off] = True
        assert int(k_mask.sum()) == T * hkv * D and int(v_mask.sum()) == T * hkv * D
        assert torch.equal(bits(kc)[~k_mask], bits(kc0)[~k_mask]), what + ": k_cache outside the slots changed"
        assert torch.equal(bits(vc)[~v_mask], bits(vc0)[~v_mask]), what + ": v_cache outside the slots changed"
        if strided:
            assert bool(torch.isnan(buf[:, :8]).all()) and bool(torch.isnan(buf[:, 8 + width:]).all())
            assert torch.equal(bits(buf[:, 8:8 + width]), bits(qkv)), "the kernel wrote its input"


@pytest.mark.parametrize("D", [40, 80])
def test_rope_and_cache_refuses_head_dim_off_the_k_layout(D):
    """The chunk-major K layout ([D/32][BS][32]) has no place for a head_dim that is no multiple of
    32: the binding refuses it before any launch (the kernel would write into the next head's keys)."""
    hq, hkv, T = 2, 2, 3
    qkv = torch.zeros(T, (hq + 2 * hkv) * D, dtype=BF, device=DEV)
    kc = torch.zeros(2, hkv, 32, D, dtype=BF, device=DEV)
    vc = torch.zeros(2, hkv, D, 32, dtype=BF, device=DEV)
    pos = torch.zeros(T, dtype=torch.int64, device=DEV)
    slots = torch.arange(T, dtype=torch.int64, device=DEV)
    for table in (None, torch.zeros(4, D, device=DEV)):
        with pytest.raises(RuntimeError, match="chunk-major K cache layout"):
            ops.rope_and_cache(qkv, pos, table, kc, vc, slots, hq, hkv, D)
    assert not bool(kc.any()) and not bool(vc.any())


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_gemm_rope_epilogue_refuses_head_dim_off_the_k_layout(fp8):
    """The decode qkv GEMM's RoPE epilogue writes K through the same layout: same refusal (D = 48
    passed its former D % 16 check)."""
    hq, hkv, D, K = 1, 1, 48, 64
    N = (hq + 2 * hkv) * D
    x = torch.zeros(1, K, dtype=BF, device=DEV)
    q = torch.empty(1, hq, D, dtype=BF, device=DEV)
    kc = torch.zeros(2, hkv, 32, D, dtype=BF, device=DEV)
    vc = torch.zeros(2, hkv, D, 32, dtype=BF, device=DEV)
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    table = torch.zeros(4, D, device=DEV)
    nat = ops.native()
    with pytest.raises(RuntimeError, match="chunk-major K cache layout"):
        if fp8:
            nat.skinny_gemm_rope_fp8(q, x, torch.zeros(N, K, dtype=torch.uint8, device=DEV),
                                     torch.ones(N, device=DEV), 0, pos, table, kc, vc, pos, hq, hkv, D, 1e-5, None)
        else:
            nat.skinny_gemm_rope(q, x, torch.zeros(N, K, dtype=BF, device=DEV), 0, pos, table, kc, vc, pos,
                                 hq, hkv, D, 1e-5, None, None, None, 3, None)
    assert not bool(kc.any()) and not bool(vc.any())
