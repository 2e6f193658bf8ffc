"""csrc/qk_norm_rope.hip (per-head QK-norm + RoPE + paged K/V write, one wave per (token, head)) and its checks
in csrc/bindings.cpp against the fp64 oracle (ops/oracle64.py qk_norm_rope) at ``qk_norm_tol``: the 8B shape, one
KV head, GQA groups 2 and 5, half waves (head_dim 64), a workgroup with a tail wave, 1 / 3 / 37 tokens, both eps,
with and without the rotation, contiguous rows and a column slice of a NaN-filled buffer; an outlier head, an
all-zero head and a head at |x| = 2^60 (larger inputs overflow the fp32 sum of squares: outside the contract);
gammas with negative, zero and large entries; bf16 and fp8 caches; the cache elements no slot addresses; the
refusals. Each case prints its worst error / tolerance (``pytest -s``)."""
import pytest
import torch

from theroundtaible_amd import ops
from theroundtaible_amd.ops import oracle64 as o64
from theroundtaible_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
U8 = torch.uint8
_COS_SIN, _ORACLE = {}, {}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def cos_sin_table(D):
    if D not in _COS_SIN:
        _COS_SIN[D] = ref.rope_cos_sin(o64.ROPE_MAX_POS, D, o64.ROPE_THETA)
    return _COS_SIN[D]


def oracle(hq, hkv, D, T, eps, rope):
    """The case's inputs and its fp64 result, computed once and shared by the bf16 and fp8 tests (read only)."""
    key = (hq, hkv, D, T, eps, rope)
    if key not in _ORACLE:
        qkv, pos, slots, kc0, vc0 = o64.qk_norm_case(hq, hkv, D, T)
        gq, gk = o64.qk_norm_gammas(D)
        x = qkv[:, :(hq + hkv) * D].reshape(T, hq + hkv, D)
        e, mag = o64.qk_norm_rope(x, gq, gk, eps, cos_sin_table(D)[pos] if rope else None, n_q=hq)
        _ORACLE[key] = (qkv, pos, slots, kc0, vc0, gq, gk, e, o64.qk_norm_tol(e, mag))
    return _ORACLE[key]


def device_rows(qkv, strided):
    """-> (rows on the device, the buffer they are a column slice of or None)."""
    if not strided:
        return qkv.to(DEV), None
    T, width = qkv.shape
    buf = torch.full((T, width + 24), float("nan"), dtype=BF, device=DEV)
    rows = buf[:, 8:8 + width]
    rows.copy_(qkv)
    assert not rows.is_contiguous() or T == 1
    return rows, buf


def check_input_kept(qkv, qkv_d, buf):
    if buf is None:
        assert torch.equal(bits(qkv_d), bits(qkv)), "the kernel wrote its input"
        return
    width = qkv.shape[1]
    assert bool(torch.isnan(buf[:, :8]).all()) and bool(torch.isnan(buf[:, 8 + width:]).all())
    assert torch.equal(bits(buf[:, 8:8 + width]), bits(qkv)), "the kernel wrote its input"


@pytest.mark.parametrize("hq,hkv,D", o64.QKNORM_SHAPES)
@pytest.mark.parametrize("T", o64.QKNORM_T)
@pytest.mark.parametrize("rope", [True, False], ids=["rope", "norope"])
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "column_slice"])
def test_qk_norm_rope_and_cache(hq, hkv, D, T, rope, strided):
    table = cos_sin_table(D).to(DEV) if rope else None
    for eps in o64.QKNORM_EPS:
        qkv, pos, slots, kc0, vc0, gq, gk, e, tol = oracle(hq, hkv, D, T, eps, rope)
        qkv_d, buf = device_rows(qkv, strided)
        kc, vc = kc0.to(DEV), vc0.to(DEV)
        q = ops.qk_norm_rope_and_cache(qkv_d, gq.to(DEV), gk.to(DEV), eps, pos.to(DEV), table, kc, vc, slots.to(DEV),
                                       hq, hkv, D)
        assert q.shape == (T, hq, D) and q.dtype == BF
        kc, vc = kc.cpu(), vc.cpu()
        what = f"qk_norm_rope_and_cache {(hq, hkv, D)} T={T} eps={eps} rope={rope} strided={strided}"
        k_written = ref.k_rows(kc, torch.arange(o64.ROPE_BLOCKS))[slots]            # [T, hkv, D]
        print(f"RATIO qk_norm.q {what} {o64.assert_within(q, e[:, :hq], tol[:, :hq], what + ' q'):.3f}")
        print(f"RATIO qk_norm.k {what} {o64.assert_within(k_written, e[:, hq:], tol[:, hq:], what + ' k'):.3f}")
        assert bool((k_written[0, hkv - 1].float() == 0).all()), what + ": the all-zero head is not exactly zero"
        assert bool(torch.isfinite(q.float()).all()) and bool(torch.isfinite(k_written.float()).all())

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
        check_input_kept(qkv, qkv_d, buf)


@pytest.mark.parametrize("hq,hkv,D", o64.QKNORM_SHAPES)
@pytest.mark.parametrize("T", o64.QKNORM_T)
@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("rope", [True, False], ids=["rope", "norope"])
def test_qk_norm_rope_and_cache_fp8(hq, hkv, D, T, scale, rope):
    """fp8 cache: q inside the tolerance, K within half an e4m3 step plus the tolerance (the bound of
    test_kv_fp8_gpu.py::test_writer_with_rope_within_half_a_step), V and every untouched byte exact."""
    table = cos_sin_table(D).to(DEV) if rope else None
    g = torch.Generator().manual_seed(3)
    k0 = torch.randint(0, 256, (o64.ROPE_BLOCKS, hkv, o64.ROPE_BS, D), dtype=U8, generator=g)
    v0 = torch.randint(0, 256, (o64.ROPE_BLOCKS, hkv, D, o64.ROPE_BS), dtype=U8, generator=g)
    blocks = torch.arange(o64.ROPE_BLOCKS)
    for eps, strided in zip(o64.QKNORM_EPS, (False, True)):
        qkv, pos, slots, _, _, gq, gk, e, t = oracle(hq, hkv, D, T, eps, rope)
        qkv_d, buf = device_rows(qkv, strided)
        kc, vc = k0.to(DEV), v0.to(DEV)
        q = ops.qk_norm_rope_and_cache(qkv_d, gq.to(DEV), gk.to(DEV), eps, pos.to(DEV), table, kc, vc, slots.to(DEV),
                                       hq, hkv, D, scale, scale)
        kc, vc = kc.cpu(), vc.cpu()
        what = f"qk_norm_rope_and_cache fp8 {(hq, hkv, D)} T={T} eps={eps} rope={rope} scale={scale}"
        print(f"RATIO qk_norm8.q {what} {o64.assert_within(q, e[:, :hq], t[:, :hq], what + ' q'):.3f}")
        kv = ref.kv_fp8_value(ref.k_rows_fp8(kc, blocks)[slots], scale).double()
        ek, tk = e[:, hq:], t[:, hq:]
        xm = ek.abs() / scale + tk / scale
        assert float(xm.max()) < ref.KV_FP8_MAX, "the inputs must stay below the e4m3 range: the bound has no saturation"
        step = torch.exp2(torch.floor(torch.log2(xm.clamp_min(2.0 ** -60))).clamp_min(-6.0) - 3.0)
        bound = 0.5 * step * scale + tk
        r = o64.assert_within(kv, ek, bound, what + " k", dtype=torch.float64)
        print(f"RATIO qk_norm8.k {what} {r:.3f}")
        v = qkv[:, (hq + hkv) * D:].reshape(T, hkv, D).float()
        assert torch.equal(ref.v_rows_fp8(vc, blocks)[slots], ref.kv_fp8_code(v, ref.kv_fp8_inv(scale))), what + ": v"
        blk, off = slots // o64.ROPE_BS, slots % o64.ROPE_BS
        k_mask, v_mask = torch.zeros(kc.shape, dtype=torch.bool), torch.zeros(vc.shape, dtype=torch.bool)
        ref.k_blocks_fp8(k_mask)[blk, :, :, off, :] = True
        ref.v_blocks_fp8(v_mask)[blk, :, :, :, off // 8, :, off % 8] = True
        assert int(k_mask.sum()) == T * hkv * D and int(v_mask.sum()) == T * hkv * D
        assert torch.equal(kc[~k_mask], k0[~k_mask]) and torch.equal(vc[~v_mask], v0[~v_mask]), what + ": untouched bytes"
        check_input_kept(qkv, qkv_d, buf)


def test_fp8_cache_equals_the_reference_byte_for_byte_without_rope():
    """No rotation and unit gammas on exact inputs (every head +-2^k: the norm is an exact power of two when
    eps = 0): kernel and reference agree on every cache byte."""
    hq, hkv, D, T = 4, 2, 128, 5
    g = torch.Generator().manual_seed(9)
    sign = torch.where(torch.rand(T, (hq + 2 * hkv) * D, generator=g) < 0.5, -1.0, 1.0)
    qkv = (sign * 2.0 ** torch.randint(-3, 4, (T, hq + 2 * hkv, 1), generator=g).float().expand(-1, -1, D)
           .reshape(T, -1)).to(BF)
    ones = torch.ones(D, dtype=BF)
    pos, slots = torch.zeros(T, dtype=torch.int64), torch.randperm(96, generator=g)[:T]
    kr, vr = torch.zeros(3, hkv, 32, D, dtype=U8), torch.zeros(3, hkv, D, 32, dtype=U8)
    q_r = ref.qk_norm_rope_and_cache(qkv, ones, ones, 0.0, pos, None, kr, vr, slots, hq, hkv, D, 0.37, 0.37)
    kc, vc = torch.zeros_like(kr, device=DEV), torch.zeros_like(vr, device=DEV)
    q = ops.qk_norm_rope_and_cache(qkv.to(DEV), ones.to(DEV), ones.to(DEV), 0.0, pos.to(DEV), None, kc, vc,
                                   slots.to(DEV), hq, hkv, D, 0.37, 0.37)
    assert torch.equal(kc.cpu(), kr) and torch.equal(vc.cpu(), vr) and torch.equal(bits(q), bits(q_r))
    assert torch.equal(q_r.float().abs(), torch.ones(T, hq, D))


def test_no_tokens_is_a_no_op():
    hq, hkv, D = 4, 1, 128
    gq, gk = (t.to(DEV) for t in o64.qk_norm_gammas(D))
    empty = torch.empty(0, dtype=torch.int64, device=DEV)
    for dt in (BF, U8):
        kc, vc = torch.ones(2, hkv, 32, D, device=DEV).to(dt), torch.ones(2, hkv, D, 32, device=DEV).to(dt)
        q = ops.qk_norm_rope_and_cache(torch.empty(0, (hq + 2 * hkv) * D, dtype=BF, device=DEV), gq, gk, 1e-6, empty,
                                       cos_sin_table(D).to(DEV), kc, vc, empty, hq, hkv, D)
        assert q.shape == (0, hq, D) and bool((kc == 1).all()) and bool((vc == 1).all())


def test_refusals_leave_the_caches_untouched():
    hq, hkv, D, T = 4, 1, 128, 3
    qkv = torch.ones(T, (hq + 2 * hkv) * D, dtype=BF, device=DEV)
    gq, gk = (t.to(DEV) for t in o64.qk_norm_gammas(D))
    pos = torch.zeros(T, dtype=torch.int64, device=DEV)
    slots = torch.arange(T, dtype=torch.int64, device=DEV)
    table = cos_sin_table(D).to(DEV)
    kc, vc = torch.zeros(2, hkv, 32, D, dtype=BF, device=DEV), torch.zeros(2, hkv, D, 32, dtype=BF, device=DEV)
    k8, v8 = torch.zeros(2, hkv, 32, D, dtype=U8, device=DEV), torch.zeros(2, hkv, D, 32, dtype=U8, device=DEV)

    def call(**kw):
        a = dict(qkv=qkv, gq=gq, gk=gk, eps=1e-6, pos=pos, table=table, kc=kc, vc=vc, slots=slots, hq=hq, hkv=hkv, D=D,
                 ks=1.0, vs=1.0)
        a.update(kw)
        return ops.qk_norm_rope_and_cache(a["qkv"], a["gq"], a["gk"], a["eps"], a["pos"], a["table"], a["kc"], a["vc"],
                                          a["slots"], a["hq"], a["hkv"], a["D"], a["ks"], a["vs"])

    bad = [
        ("gamma length", RuntimeError, dict(gq=gq[:64].contiguous())),
        ("gamma length", RuntimeError, dict(gk=torch.cat([gk, gk]))),
        ("gamma dtype", RuntimeError, dict(gq=gq.float())),
        ("gamma dtype", RuntimeError, dict(gk=gk.float())),
        ("bf16 K with uint8 V", (RuntimeError, ValueError), dict(vc=v8)),
        ("uint8 K with bf16 V", (RuntimeError, ValueError), dict(kc=k8)),
        ("negative eps", RuntimeError, dict(eps=-1e-6)),
        ("NaN eps", RuntimeError, dict(eps=float("nan"))),
        ("fp8 scale 0", RuntimeError, dict(kc=k8, vc=v8, ks=0.0)),
        ("fp8 scale inf", RuntimeError, dict(kc=k8, vc=v8, vs=float("inf"))),
        ("positions dtype", RuntimeError, dict(pos=pos.int())),
        ("slots count", RuntimeError, dict(slots=slots[:2])),
        ("qkv width", RuntimeError, dict(hq=hq + 1)),
        ("table width", RuntimeError, dict(table=cos_sin_table(64).to(DEV))),
    ]
    for name, exc, kw in bad:
        with pytest.raises(exc):
            call(**kw)
        torch.cuda.synchronize()
        assert not bool(kc.any()) and not bool(vc.any()) and not bool(k8.any()) and not bool(v8.any()), name
    # the bindings themselves refuse a mixed pair too (ops.qk_norm_rope_and_cache stops it one level up)
    q = torch.zeros(T, hq, D, dtype=BF, device=DEV)
    for name, fn, a, b in (("qk_norm_rope_and_cache", ops.native().qk_norm_rope_and_cache, kc, v8),
                           ("qk_norm_rope_and_cache_fp8", ops.native().qk_norm_rope_and_cache_fp8, k8, vc),
                           ("qk_norm_rope_and_cache_fp8", ops.native().qk_norm_rope_and_cache_fp8, kc, vc),
                           ("qk_norm_rope_and_cache", ops.native().qk_norm_rope_and_cache, k8, v8)):
        with pytest.raises(RuntimeError):
            fn(q, qkv, gq, gk, 1e-6, pos, table, a, b, slots, hq, hkv, D)
        torch.cuda.synchronize()
        assert not bool(kc.any()) and not bool(vc.any()) and not bool(k8.any()) and not bool(v8.any()), name
    # head dims the one-wave-per-head mapping does not take
    for d in (32, 256):
        w = torch.ones(T, (hq + 2 * hkv) * d, dtype=BF, device=DEV)
        kcd, vcd = torch.zeros(2, hkv, 32, d, dtype=BF, device=DEV), torch.zeros(2, hkv, d, 32, dtype=BF, device=DEV)
        g = torch.ones(d, dtype=BF, device=DEV)
        with pytest.raises(RuntimeError, match="head_dim must be 64 or 128"):
            call(qkv=w, gq=g, gk=g, kc=kcd, vc=vcd, D=d, table=None)
        assert not bool(kcd.any()) and not bool(vcd.any())
    assert call().shape == (T, hq, D) and bool(kc.any()) and bool(vc.any())       # and the good call goes through
