"""The FP8 K/V cache (kv_dtype "fp8") on the GPU: every cache writer (K2 rope_cache.hip, the ROPE epilogue of the
decode GEMMs on bf16 / fp8 / mxfp4 weights) byte for byte or within half an e4m3 step of ops/reference.py, decode
attention (csrc/attn_core.h Tile8) and the 32x32 prefill kernel (+ key split) against the fp64 oracle of the fp8
twins with the unchanged ``attn_tol``, the K8 block copy on a byte pool, and the engine end to end."""
import functools

import pytest
import torch

from test_engine_gpu import _shared_turns
from theroundtaible_amd import ops
from theroundtaible_amd.engine import Engine, EngineConfig, SamplingParams, Turn
from theroundtaible_amd.errors import ConfigError
from theroundtaible_amd.ops import oracle64 as o64
from theroundtaible_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
U8 = torch.uint8


# ---- writers ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_writer_every_finite_bf16_byte_exact(scale):
    """K2 without RoPE: all 65 280 finite bf16 patterns through the K and the V columns of a
    (hq, hkv, d) = (2, 1, 128) row, 510 tokens; the caches equal the reference byte for byte."""
    hq, hkv, d = 2, 1, 128
    y = o64.finite_bf16_table()
    T = y.numel() // d
    assert T * d == 65280
    qkv = torch.zeros(T, (hq + 2 * hkv) * d, dtype=BF)
    qkv[:, hq * d:(hq + 1) * d] = y.reshape(T, d)
    qkv[:, (hq + 1) * d:] = y.flip(0).reshape(T, d)
    nb = (T + 31) // 32 + 1
    g = torch.Generator().manual_seed(11)
    slots = torch.randperm(nb * 32, generator=g)[:T]
    pos = torch.zeros(T, dtype=torch.int64)
    kc, vc = torch.zeros(nb, hkv, 32, d, dtype=U8, device=DEV), torch.zeros(nb, hkv, d, 32, dtype=U8, device=DEV)
    q = ops.rope_and_cache(qkv.to(DEV), pos.to(DEV), None, kc, vc, slots.to(DEV), hq, hkv, d, scale, scale)
    kr, vr = torch.zeros(nb, hkv, 32, d, dtype=U8), torch.zeros(nb, hkv, d, 32, dtype=U8)
    ref.rope_and_cache(qkv, pos, None, kr, vr, slots, hq, hkv, d, scale, scale)
    assert torch.equal(kc.cpu(), kr) and torch.equal(vc.cpu(), vr)
    # (a quarter of the bf16 patterns lie below half the smallest e4m3 step and give the zero codes)
    assert int(kr.count_nonzero()) > 40000 and torch.equal(q.cpu(), qkv[:, :hq * d].reshape(T, hq, d))


@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_writer_with_rope_within_half_a_step(scale):
    hq, hkv, D, T = 4, 1, 128, 33
    qkv, pos, slots, _, _ = o64.rope_case(hq, hkv, D, T)
    table = ref.rope_cos_sin(o64.ROPE_MAX_POS, D, o64.ROPE_THETA)
    kc = torch.zeros(o64.ROPE_BLOCKS, hkv, 32, D, dtype=U8, device=DEV)
    vc = torch.zeros(o64.ROPE_BLOCKS, hkv, D, 32, dtype=U8, device=DEV)
    q = ops.rope_and_cache(qkv.to(DEV), pos.to(DEV), table.to(DEV), kc, vc, slots.to(DEV), hq, hkv, D, scale, scale)
    x = qkv[:, :(hq + hkv) * D].reshape(T, hq + hkv, D)
    e, mag = o64.rope(x, table[pos])
    t = o64.rope_tol(e, mag)
    o64.assert_within(q, e[:, :hq], t[:, :hq], "q stays bf16")
    blocks = torch.arange(o64.ROPE_BLOCKS)
    kv = ref.kv_fp8_value(ref.k_rows_fp8(kc.cpu(), blocks)[slots], scale).double()
    ek, tk = e[:, hq:], t[:, hq:]
    xm = ek.abs() / scale + tk / scale
    step = torch.exp2(torch.floor(torch.log2(xm.clamp_min(2.0 ** -60))).clamp_min(-6.0) - 3.0)
    bound = 0.5 * step * scale + tk
    r = o64.assert_within(kv, ek, bound, f"fp8 K after RoPE, scale {scale}", dtype=torch.float64)
    print(f"fp8 K after RoPE scale {scale}: error / bound {r:.3f}")
    # V is not rotated: byte-exact
    v = qkv[:, (hq + hkv) * D:].reshape(T, hkv, D).float()
    assert torch.equal(ref.v_rows_fp8(vc.cpu(), blocks)[slots], ref.kv_fp8_code(v, ref.kv_fp8_inv(scale)))


def quantise(W, wq, **kw):
    if wq == "fp8":
        return ops.shuffle_weight_fp8(W, **kw)
    if wq == "mxfp4":
        return ops.shuffle_weight_mxfp4(W, **kw)
    return ops.shuffle_weight(W, **kw), None


def dequantise(Wq, sc, wq, **kw):
    if wq == "fp8":
        return ops.unshuffle_weight_fp8(Wq, sc, **kw)
    if wq == "mxfp4":
        return ops.unshuffle_weight_mxfp4(Wq, sc, **kw)
    return ops.unshuffle_weight(Wq, **kw)


def rope_setup(M, hkv, d, seed=0):
    g = torch.Generator(device=DEV).manual_seed(100 + seed)
    positions = torch.randint(0, 4000, (M,), device=DEV, dtype=torch.int64, generator=g)
    nb = 8
    slots = torch.randperm(nb * 32, device=DEV, generator=g)[:M].to(torch.int64)
    kc = torch.zeros(nb, hkv, 32, d, dtype=U8, device=DEV)
    vc = torch.zeros(nb, hkv, d, 32, dtype=U8, device=DEV)
    return positions, slots, kc, vc


def cache_values(kc, vc, ks, vs):
    """Dequantised K, V rows [NB * 32, Hkv, D] of whole fp8 caches."""
    blocks = torch.arange(kc.shape[0])
    return (ref.kv_fp8_value(ref.k_rows_fp8(kc.cpu(), blocks), ks), ref.kv_fp8_value(ref.v_rows_fp8(vc.cpu(), blocks), vs))


@pytest.mark.parametrize("wq", ["none", "fp8", "mxfp4"])
def test_gemm_epilogue_closed_form(wq):
    """The construction of test_scale_indexing_closed_form: weight row n is the constant 2^(n mod 5),
    all-ones x, K = 64 (mxfp4's k-record is 128 deep: K = 128 of x = 1/2, the same sums): with
    k_scale = v_scale = 4 every output (64 ... 1024) is representable and the dequantised caches equal
    the reference exactly; with scale 1 the values >= 512 saturate to exactly 448."""
    K, M = (128 if wq == "mxfp4" else 64), 3
    hq, hkv, d = 2, 1, 128
    N = (hq + 2 * hkv) * d
    x = torch.full((M, K), 64.0 / K, dtype=BF, device=DEV)
    n = torch.arange(N, device=DEV)
    W = torch.exp2((n % 5).float())[:, None].expand(N, K).contiguous().to(BF)
    Wq, sc = quantise(W, wq, rope_heads=hq + hkv, head_dim=d)
    qkv = (64 * torch.exp2((n % 5).float()))[None, :].expand(M, N).contiguous().cpu()   # exact projection
    one, zero = torch.ones(64, d // 2), torch.zeros(64, d // 2)
    for cs in (torch.cat([one, zero], 1), torch.cat([zero, one], 1)):
        for s in (4.0, 1.0):
            positions, slots, kc, vc = rope_setup(M, hkv, d)
            positions = positions % 64
            q = ops.skinny_gemm_rope(x, Wq, ops.PRO_PLAIN, positions, cs.to(DEV), kc, vc, slots, hq, hkv, d,
                                     wscale=sc, k_scale=s, v_scale=s)
            kr, vr = torch.zeros_like(kc).cpu(), torch.zeros_like(vc).cpu()
            q_r = ref.rope_and_cache(qkv, positions.cpu(), cs, kr, vr, slots.cpu(), hq, hkv, d, s, s)
            assert torch.equal(q.float().cpu(), q_r.to(BF).float())
            assert torch.equal(kc.cpu(), kr) and torch.equal(vc.cpu(), vr)
            kv, vv = cache_values(kc, vc, s, s)
            sl = slots.cpu()
            want_v = qkv[:, (hq + hkv) * d:].reshape(M, hkv, d)
            if s == 4.0:
                assert torch.equal(vv[sl], want_v)                          # representable: exact
                assert torch.equal(kv[sl].abs().sort(-1).values,
                                   qkv[:, hq * d:(hq + hkv) * d].reshape(M, hkv, d).abs().sort(-1).values)
            else:
                assert torch.equal(vv[sl], want_v.clamp(max=448.0)) and float(vv.max()) == 448.0
                assert float(kv.abs().max()) == 448.0


@pytest.mark.parametrize("wq", ["none", "fp8", "mxfp4"])
@pytest.mark.parametrize("M,hq,hkv,d,bias", [(1, 32, 8, 128, False), (3, 4, 1, 128, True), (20, 4, 1, 128, True)])
def test_gemm_epilogue_random(M, hq, hkv, d, bias, wq):
    """The shapes of test_skinny_gemm_rope_fp8; its close(., 0.05, 0.02) widened by half an e4m3 step:
    rtol + 2^-4, atol + 2^-10 * scale. Three calls are bit-identical."""
    K = 512
    N = (hq + 2 * hkv) * d
    g = torch.Generator(device=DEV)
    rnd = lambda seed, *shape, scale=1.0: (torch.randn(*shape, generator=g.manual_seed(seed), device=DEV) * scale).to(BF)  # noqa: E731
    x, W, gam = rnd(61, M, K), rnd(62, N, K, scale=0.05), rnd(63, K)
    b = rnd(64, N, scale=0.5) if bias else None
    cos_sin = ref.rope_cos_sin(4096, d, 500000.0, DEV)
    positions, slots, kc, vc = rope_setup(M, hkv, d, seed=M)
    kw = dict(rope_heads=hq + hkv, head_dim=d)
    Wq, sc = quantise(W, wq, gamma=gam, **kw)
    ks, vs = 0.5, 0.25
    runs = []
    for _ in range(3):
        kc.zero_()
        vc.zero_()
        q = ops.skinny_gemm_rope(x, Wq, ops.PRO_NORM, positions, cos_sin, kc, vc, slots, hq, hkv, d, 1e-5,
                                 bias=ops.rope_bias(b, hq, hkv, d) if bias else None, wscale=sc, k_scale=ks, v_scale=vs)
        runs.append((q.clone(), kc.clone(), vc.clone()))
    for r in runs[1:]:
        assert all(torch.equal(a, c) for a, c in zip(runs[0], r))
    Wd = dequantise(Wq, sc, wq, **kw).cpu()                              # natural row order
    Wp = Wd[ref.rope_row_perm(N, hq + hkv, d)]
    kr = torch.zeros(kc.shape, dtype=BF)
    vr = torch.zeros(vc.shape, dtype=BF)
    q_r = ref.skinny_gemm_rope(x.cpu(), Wp, 1, positions.cpu(), cos_sin.cpu(), kr, vr, slots.cpu(), hq, hkv, d,
                               1e-5, bias=ops.rope_bias(b.cpu(), hq, hkv, d) if bias else None)

    def close(a, e, atol, rtol):
        dd = (a.float() - e.float()).abs()
        assert bool((dd <= atol + rtol * e.float().abs()).all()), f"max err {dd.max().item():.4g}"
    close(runs[0][0].cpu(), q_r, 0.05, 0.02)
    kv, vv = cache_values(kc, vc, ks, vs)
    blocks = torch.arange(kc.shape[0])
    k_ref = ref.k_rows(kr, blocks).float()
    v_ref = vr[blocks].permute(0, 3, 1, 2).reshape(-1, hkv, d).float()
    close(kv, k_ref, 0.05 + 2.0 ** -10 * ks, 0.02 + 2.0 ** -4)
    close(vv, v_ref, 0.05 + 2.0 ** -10 * vs, 0.02 + 2.0 ** -4)
    assert float(kv.abs().max()) > 0.5 and float(vv.abs().max()) > 0.5


def test_bindings_refuse_mixed_and_wrong_caches():
    q = torch.zeros(1, 8, 128, dtype=BF, device=DEV)
    k8, v8 = torch.zeros(2, 1, 32, 128, dtype=U8, device=DEV), torch.zeros(2, 1, 128, 32, dtype=U8, device=DEV)
    vb = torch.zeros(2, 1, 128, 32, dtype=BF, device=DEV)
    bt, cl = torch.zeros(1, 2, dtype=torch.int32, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="mixed"):
        ops.paged_attention_decode(q, k8, vb, bt, cl, 0.1)
    ws = ops.DecodeWorkspace(1, 8, 128, 1, DEV)
    nat = ops.native()
    with pytest.raises(RuntimeError, match="one dtype|mixed"):
        nat.paged_attention_decode_fp8(q, q, k8, vb, bt, cl, 0.1, 1, ws.partial_o, ws.partial_ml, ws.counters)
    with pytest.raises(RuntimeError, match="scale"):
        ops.paged_attention_decode(q, k8, v8, bt, cl, 0.1, 1, ws, k_scale=0.0)
    q64 = torch.zeros(1, 4, 64, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="head_dim 128"):
        ops.paged_attention_decode(q64, torch.zeros(2, 1, 32, 64, dtype=U8, device=DEV),
                                   torch.zeros(2, 1, 64, 32, dtype=U8, device=DEV), bt, cl, 0.1)
    # a GQA group > 8 would take the 16x16 prefill kernel: refused, not run
    q16 = torch.zeros(4, 16, 128, dtype=BF, device=DEV)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="group"):
        ops.prefill_attention(q16, k8, v8, bt, cu, torch.zeros(1, dtype=torch.int32, device=DEV), 0.1)


# ---- attention against the fp64 oracle of the fp8 twins -------------------------------------------------

class OnDevice:
    def __init__(self, twin, prefill=False):
        self.case = twin
        self.e, self.A, self.tol = o64.attn_oracle(twin, prefill)
        self.q, self.kc, self.vc, self.bt, self.cl, self.cu, self.st = (
            t.to(DEV) for t in (twin.q, twin.k_cache, twin.v_cache, twin.block_tables, twin.ctx_lens, twin.cu_q,
                                twin.start_pos))


@functools.lru_cache(maxsize=2)
def decode_twin(kind, cfg, scales=(1.0, 1.0), lens=o64.ATTN_DECODE_LENS):
    return OnDevice(o64.attn_case_fp8(o64.attn_decode_case(kind, *cfg, lens=lens), *scales))


@functools.lru_cache(maxsize=2)
def group_twin(kind, cfg, scales=(1.0, 1.0)):
    return OnDevice(o64.attn_case_fp8(o64.attn_group_case(kind, *cfg), *scales))


@functools.lru_cache(maxsize=2)
def prefill_twin(kind, cfg, specs):
    return OnDevice(o64.attn_case_fp8(o64.attn_case(kind, *cfg, specs), 0.5, 4.0), prefill=True)


def check_decode(c, splits, what, grouped=False):
    """One launch within the tolerance; a second launch on the same workspace and the planned launch
    reproduce it bit for bit and leave the arrival counters at zero."""
    case = c.case
    hq, hkv, d = case.hq, case.hkv, case.d
    G = hq // hkv
    B = c.q.shape[0]
    sc = dict(k_scale=case.k_scale, v_scale=case.v_scale)
    groups = None
    if grouped:
        table, nmax = ops.decode_groups(case.group_of, case.shared, G)
        assert nmax <= max(1, 16 // G)
        groups = table.to(DEV)
    ws = ops.DecodeWorkspace(B, hq, d, splits, DEV, max_group=16 // G if grouped else 1)
    out = ops.paged_attention_decode(c.q, c.kc, c.vc, c.bt, c.cl, case.scale, splits, ws, groups=groups, **sc)
    r = o64.assert_within(out, c.e, c.tol, what)
    print(f"{what}: error / tolerance {r:.3f}")
    again = ops.paged_attention_decode(c.q, c.kc, c.vc, c.bt, c.cl, case.scale, splits, ws, groups=groups, **sc)
    assert torch.equal(out, again)
    assert int(ws.counters.abs().sum()) == 0
    assert ops.attn_plan(c.bt, c.cl, splits, ws, hq, hkv, groups, B)
    planned = ops.paged_attention_decode(c.q, c.kc, c.vc, c.bt, c.cl, case.scale, splits, ws, groups=groups,
                                         planned=True, **sc)
    assert torch.equal(out, planned)
    assert int(ws.counters.abs().sum()) == 0
    return r


DECODE_CFGS = ((8, 1, 128), (32, 8, 128), (28, 4, 128))      # copy loop + GM 8; ping-pong + GM 4; G = 7
# splits 1 / 3 / 8 everywhere, plus 64 (most items empty) for (8, 1, 128)
DECODE_CFG_SPLITS = [(cfg, s) for cfg in DECODE_CFGS for s in (1, 3, 8) + ((64,) if cfg == (8, 1, 128) else ())]


@pytest.mark.parametrize("kind", o64.ATTN_KINDS)
@pytest.mark.parametrize("cfg,splits", DECODE_CFG_SPLITS)
def test_decode(cfg, splits, kind):
    check_decode(decode_twin(kind, cfg), splits, f"fp8 decode {cfg} {kind} splits {splits}")


SCALED = ((0.5, 4.0), (0.37, 2.9))       # every (8, 1, 128) decode case again at non-unit scales


@pytest.mark.parametrize("scales", SCALED)
@pytest.mark.parametrize("splits", (1, 3, 8, 64))
@pytest.mark.parametrize("kind", o64.ATTN_KINDS)
def test_decode_scaled(kind, splits, scales):
    """One split: the launch's own store folds v_scale; more: decode_combine_kernel does."""
    check_decode(decode_twin(kind, (8, 1, 128), scales), splits, f"fp8 decode (8, 1, 128) {kind} {scales} splits {splits}")


@pytest.mark.parametrize("scales", ((1.0, 1.0),) + SCALED)
@pytest.mark.parametrize("splits", (1, 2))
def test_decode_refill_and_plan_row_boundary(splits, scales):
    check_decode(decode_twin("census", (8, 1, 128), scales, o64.ATTN_REFILL_LENS), splits,
                 f"fp8 refill census {scales} splits {splits}")


@pytest.mark.parametrize("splits", (1, 3, 10))
@pytest.mark.parametrize("kind", o64.ATTN_KINDS)
@pytest.mark.parametrize("cfg", ((32, 8, 128), (8, 1, 128)))
def test_grouped_decode(cfg, kind, splits):
    """Shared-prefix groups (GM 16; at one split the groups' members are combined inside the launch)."""
    check_decode(group_twin(kind, cfg), splits, f"fp8 grouped {cfg} {kind} splits {splits}", grouped=True)


@pytest.mark.parametrize("scales", SCALED)
@pytest.mark.parametrize("splits", (1, 3, 10))
@pytest.mark.parametrize("kind", o64.ATTN_KINDS)
def test_grouped_decode_scaled(kind, splits, scales):
    """Groups of (8, 1, 128) at non-unit scales. At one split a group's two members are merged by the
    last-arriving workgroup INSIDE the launch: the only default-knob route to that combine's v_scale fold
    (two or more splits take decode_combine_kernel), so with v_scale = 1 alone the fold could be deleted
    unnoticed."""
    c = group_twin(kind, (8, 1, 128), scales)
    if splits == 1:
        table, nmax = ops.decode_groups(c.case.group_of, c.case.shared, 8)
        assert nmax == 2                         # some row really is combined in the launch
    check_decode(c, splits, f"fp8 grouped (8, 1, 128) {kind} {scales} splits {splits}", grouped=True)


@pytest.mark.parametrize("kind", o64.ATTN_KINDS)
@pytest.mark.parametrize("cfg", ((32, 8, 128), (28, 4, 128), (12, 4, 128), (16, 1, 128)))
def test_prefill(cfg, kind):
    """The 32x32 kernel over fp8 pages (padded head slots at G = 7 and 3) at scales (0.5, 4). (16, 1, 128)
    is a GQA group of 16: the 16x16 fallback it would take has no fp8 form, so that shape must be refused."""
    c = prefill_twin(kind, cfg, o64.ATTN_PREFILL_SPECS)
    if cfg == (16, 1, 128):          # G = 16 would take the 16x16 kernel, which has no fp8 form: refused
        with pytest.raises(RuntimeError, match="group"):
            ops.prefill_attention(c.q, c.kc, c.vc, c.bt, c.cu, c.st, c.case.scale, k_scale=0.5, v_scale=4.0)
        return
    out = ops.prefill_attention(c.q, c.kc, c.vc, c.bt, c.cu, c.st, c.case.scale, k_scale=0.5, v_scale=4.0)
    r = o64.assert_within(out, c.e, c.tol, f"fp8 prefill {cfg} {kind}")
    print(f"fp8 prefill {cfg} {kind}: error / tolerance {r:.3f}")
    assert torch.equal(out, ops.prefill_attention(c.q, c.kc, c.vc, c.bt, c.cu, c.st, c.case.scale, k_scale=0.5,
                                                  v_scale=4.0))


@pytest.mark.parametrize("kind", o64.ATTN_KINDS)
@pytest.mark.parametrize("cfg", ((4, 1, 128), (32, 8, 128)))
def test_prefill_key_split(cfg, kind):
    c = prefill_twin(kind, cfg, o64.ATTN_SPLIT_SPECS)
    case = c.case
    rows = ops.native().prefill_rows_per_tile(case.hq // case.hkv, case.d)
    plan = ops.prefill_split_plan(case.cu_q, rows, case.start_pos, case.hkv, num_cus=1 << 20, min_chunk_tiles=1)
    assert plan is not None and plan[2] >= 2
    split = (plan[0].to(DEV), plan[1].to(DEV), plan[2])
    what = f"fp8 key split {cfg} {kind}"
    sc = dict(k_scale=0.5, v_scale=4.0)
    out = ops.prefill_attention(c.q, c.kc, c.vc, c.bt, c.cu, c.st, case.scale, split=split, **sc)
    r = o64.assert_within(out, c.e, c.tol, what)
    print(f"{what}: error / tolerance {r:.3f}")
    whole = ops.prefill_attention(c.q, c.kc, c.vc, c.bt, c.cu, c.st, case.scale, **sc)
    o64.assert_within(whole, c.e, c.tol, what + " whole tiles")
    o64.assert_within(out, whole.cpu().double(), 2 * c.tol, what + " vs whole tiles")
    assert torch.equal(out, ops.prefill_attention(c.q, c.kc, c.vc, c.bt, c.cu, c.st, case.scale, split=split, **sc))


def test_block_copy_on_an_fp8_pool():
    L, nb, elems = 2, 6, 1 * 32 * 128
    g = torch.Generator().manual_seed(5)
    k = torch.randint(0, 256, (L, nb, elems), dtype=U8, generator=g).to(DEV)
    v = torch.randint(0, 256, (L, nb, elems), dtype=U8, generator=g).to(DEV)
    k0, v0 = k.clone(), v.clone()
    ops.kv_block_copy(k, v, [1, 4], [3, 0])
    for t, t0 in ((k, k0), (v, v0)):
        assert torch.equal(t[:, 3], t0[:, 1]) and torch.equal(t[:, 0], t0[:, 4])
        assert torch.equal(t[:, [1, 2, 4, 5]], t0[:, [1, 2, 4, 5]])


# ---- engine -------------------------------------------------------------------------------------------

def fp8kv_engine(model, **kw):
    cfg = dict(model=model, weights="random-full:5", device=DEV, num_blocks=64, kv_dtype="fp8",
               kv_scale={"k": 0.5, "v": [2.0, 0.25]})
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


@pytest.mark.parametrize("model", ["tiny-llama-128", "tiny-qwen-128"])
def test_fused_decode_matches_unfused(model):
    """Both paths write and read the same fp8 pool: the bound of test_fp8_fused_decode_matches_unfused."""
    from theroundtaible_amd.models.llama import AttnMeta
    e = fp8kv_engine(model, use_graphs=False)
    assert e.kv.k.dtype == U8 and e.kv_dtype == "fp8"
    ids = e.encode_prompt("fused versus unfused decode " * 4)
    seqs = [e.kv.seq("a"), e.kv.seq("b")]
    e.prefill([(seqs[0], ids), (seqs[1], ids[:-3])])
    for s in seqs:
        e.kv.ensure_capacity(s, s.length + 1)
    pos = torch.tensor([s.length for s in seqs], device=DEV)
    slots = torch.tensor([s.blocks[p // 32] * 32 + p % 32 for s, p in zip(seqs, pos.tolist())], device=DEV)
    bt = torch.zeros(2, 8, dtype=torch.int32)
    for j, s in enumerate(seqs):
        bt[j, :len(s.blocks)] = torch.tensor(s.blocks)
    meta = AttnMeta("decode", slots, bt.to(DEV), (pos + 1).to(torch.int32), num_splits=4)
    tok = torch.tensor([5, 7], device=DEV)
    assert e.model.fused_decode_ok(tok)
    fused = e.model.forward(tok, pos, e.kv, meta).float()
    e.model.use_fused = False
    plain = e.model.forward(tok, pos, e.kv, meta).float()
    cos = torch.nn.functional.cosine_similarity(fused, plain, dim=-1)
    print(f"fp8 KV fused vs unfused cosine min = {float(cos.min())}")
    assert float(cos.min()) > 0.999


@pytest.mark.parametrize("model", ["tiny-llama-128", "tiny-qwen-128"])
def test_prefill_logits_match_cpu(model):
    g = fp8kv_engine(model, use_graphs=False)
    c = fp8kv_engine(model, device="cpu", dtype="fp32", num_blocks=512)
    ids = g.encode_prompt("De ridders van de ronde tafel bespreken de architectuur van de cache-laag. " * 3)
    lg = g.prefill([(g.kv.seq("a"), ids)]).float().cpu()
    lc = c.prefill([(c.kv.seq("a"), ids)]).float()
    cos = torch.nn.functional.cosine_similarity(lg, lc, dim=-1)
    print(f"GPU vs CPU fp8-KV prefill cosine min = {float(cos.min())}")
    assert float(cos.min()) > 0.99


@pytest.mark.parametrize("model", ["tiny-llama-128", "tiny-qwen-128"])
def test_engine_graphs_deterministic(model):
    sp = SamplingParams(temperature=0.0, max_new_tokens=24, ignore_eos=True, stop_on_consensus=False)
    outs = []
    for _ in range(2):
        e = fp8kv_engine(model)
        assert e.ecfg.use_graphs
        r = e.run_turns([Turn("a", "determinisme met acht-bits sleutels", sp), Turn("b", "nog een", sp)])
        assert all(t.error is None and len(t.ids) == 24 for t in r)
        outs.append([t.ids for t in r])
    assert outs[0] == outs[1]


@pytest.mark.parametrize("wq", ["none", "fp8", "mxfp4"])
def test_three_knights_share_a_prefix_through_a_group(wq):
    a = fp8kv_engine("tiny-llama-128", num_blocks=512, weight_quant=wq, use_graphs=True)
    b = fp8kv_engine("tiny-llama-128", num_blocks=512, weight_quant=wq, use_graphs=False)
    _, ta = _shared_turns([], 1)
    _, tb = _shared_turns([], 1)
    oa, ob = a.run_turns(ta), b.run_turns(tb)
    assert all(o.error is None and o.metrics["shared_tokens"] > 0 for o in oa + ob)
    assert [o.ids for o in oa] == [o.ids for o in ob]


def test_refusal_and_pool_size_on_gpu():
    with pytest.raises(ConfigError, match="kv_dtype.*bf16"):
        Engine(EngineConfig(model="tiny-llama-128", device=DEV, dtype="fp16", kv_dtype="fp8"))
    mk = lambda kvd: Engine(EngineConfig(model="tiny-llama-128", device=DEV, kv_dtype=kvd, kv_budget_bytes=64 << 20,   # noqa: E731
                                         weights="random:1"))
    a, b = mk("bf16"), mk("fp8")
    assert b.kv_capacity_tokens == 2 * a.kv_capacity_tokens
    assert b.kv.k.numel() * b.kv.k.element_size() == a.kv.k.numel() * a.kv.k.element_size()
