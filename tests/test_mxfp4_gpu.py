"""MXFP4 weight-only decode GEMMs on the GPU (csrc/gemm_skinny_fp4.hip, the WT_FP4 paths of
csrc/skinny_core.h): the hardware convert's semantics, the quantiser against the CPU contract with 0
differences, scale indexing in closed form, every prologue x epilogue, the RoPE epilogue, the engine
paths and residency.

Dequantisation is exact (every value(code) * 2^(e-127) is a bf16 value), so the GEMM oracle is
ref.skinny_gemm / ref.skinny_gemm_rope on the dequantised weight and the tolerances are those
tests/test_gemm_gpu.py uses for the same epilogues. The GPU arrays are compared byte for byte with
the CPU reference's through ``gpu_layout`` below, a statement of the record layout in index
arithmetic that shares no code with csrc/skinny_core.h."""
import pytest
import torch

from test_mxfp4_cpu import hand_blocks
from theroundtaible_amd import ops
from theroundtaible_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
SCALE_BYTES = (2, 100, 127, 140, 252)


def bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(torch.bfloat16)


def close(a, b, atol, rtol=0.0):
    d = (a.float() - b.float()).abs()
    tol = atol + rtol * b.float().abs()
    assert bool((d <= tol).all()), f"max err {d.max().item():.4g}"


def record_order(N, K, rope, swiglu):
    """The record order of an [N, K] weight (skinny_core.h weight_order) and the 128-deep records per
    chunk of that order for mxfp4 (0: tile-major)."""
    T, steps = (N // 2 if swiglu else N) // 16, K // 32
    order = 5 if swiglu else 3 if rope else 5 if T >= 4096 else 1 if steps >= 384 else 0
    if order and steps % (1 << (order - 1)):
        order = 0
    return order, (0 if order == 0 else 1 << max(order - 3, 0))


def gpu_layout(codes, scale, rope=False, swiglu=False):
    """Row-major codes [N, K/2] and scale bytes [N, K/32], rows in the epilogue's order, as the GPU
    holds them: record (tile t, k-step s, half h, lane l) is the 16 bytes of row 16t + (l & 15) + h N/2
    at k0 = 128 s + 32 (l >> 4), with that block's scale byte at the record's own index."""
    N, K = codes.shape[0], 2 * codes.shape[1]
    H = 2 if swiglu else 1
    T, ks = N // (16 * H), K // 128
    order, C = record_order(N, K, rope, swiglu)
    t, s, h, l = torch.meshgrid(torch.arange(T), torch.arange(ks), torch.arange(H), torch.arange(64), indexing="ij")
    first = (t * ks + s) if order == 0 else ((s // C) * T * C + t * C + s % C)
    rec = (first * H + h) * 64 + l
    row = 16 * t + (l & 15) + h * (N // 2)
    blk = 4 * s + (l >> 4)
    assert torch.equal(rec.flatten().sort().values, torch.arange(N * K // 32))
    out_c = torch.empty(N * K // 32, 16, dtype=torch.uint8)
    out_s = torch.empty(N * K // 32, dtype=torch.uint8)
    out_c[rec.flatten()] = codes.reshape(N, K // 32, 16)[row.flatten(), blk.flatten()]
    out_s[rec.flatten()] = scale[row.flatten(), blk.flatten()]
    return out_c.reshape(N, K // 2), out_s.reshape(N, K // 32)


def test_convert_semantics_exact():
    """Every code at every position of a block, under scale bytes over the whole range, through the
    GEMM's hardware convert: PLAIN / STORE with one-hot activation rows reads single weight elements
    back, which must be the dequantised values bit for bit. Pins nibble order, byte select, sign and
    the scale operand of v_cvt_scalef32_pk_bf16_fp4."""
    N, K = 48, 128
    b = torch.arange(N * K // 32)[:, None]
    c = ((torch.arange(32)[None, :] + b) % 16).to(torch.uint8).reshape(N, K // 2, 2)
    codes = (c[:, :, 0] | (c[:, :, 1] << 4)).contiguous()
    scale = torch.tensor(SCALE_BYTES, dtype=torch.uint8)[b.flatten() % 5].reshape(N, K // 32)
    W = ref.dequantize_mxfp4(codes, scale)                 # every block holds 4 and 6: the quantiser returns `scale`
    assert torch.isfinite(W.float()).all() and int((W.float() == 0).sum()) == N * K // 8
    Wq, sc = ops.shuffle_weight_mxfp4(W.to(DEV))
    want_c, want_s = gpu_layout(codes, scale)
    assert torch.equal(Wq.cpu(), want_c) and torch.equal(sc.cpu(), want_s)
    assert torch.equal(ops.unshuffle_weight_mxfp4(Wq, sc).cpu().view(torch.int16), W.view(torch.int16))
    seen = torch.zeros(N, K, dtype=torch.bool)
    for c0 in range(0, K, 16):
        x = torch.zeros(16, K, dtype=torch.bfloat16, device=DEV)
        x[torch.arange(16), c0 + torch.arange(16)] = 1.0
        got = ops.skinny_gemm(x, Wq, ops.PRO_PLAIN, ops.EPI_STORE, wscale=sc).cpu()      # [16, N]
        want = W[:, c0:c0 + 16].t().contiguous()
        # bit for bit; a zero weight (codes 0 and 8) reads back as the accumulator's +0
        same = (got.view(torch.int16) == want.view(torch.int16)) | ((want.float() == 0) & (got.view(torch.int16) == 0))
        bad = (~same).nonzero()
        assert bad.numel() == 0, (c0, bad[:8].tolist(), got[~same][:8].tolist(), want[~same][:8].tolist())
        seen[:, c0:c0 + 16] = True
    assert bool(seen.all())


QUANT_SHAPES = [(48, 128, {}), (256, 512, {}), (1024, 14336, {}),
                (6 * 128, 256, {"rope_heads": 4, "head_dim": 128}), (512, 4096, {"swiglu": True})]


@pytest.mark.parametrize("N,K,kw", QUANT_SHAPES)
def test_quantiser_equals_reference(N, K, kw):
    W = bf(N, K, scale=0.05, seed=11)
    gam = bf(K, seed=12)
    Wq, sc = ops.shuffle_weight_mxfp4(W, gam, **kw)
    assert Wq.dtype == torch.uint8 and Wq.shape == (N, K // 2) and sc.dtype == torch.uint8 and sc.shape == (N, K // 32)
    rope = {k: kw[k] for k in ("rope_heads", "head_dim") if k in kw}
    codes_r, scale_r = ref.quantize_mxfp4(W.cpu(), gam.cpu(), **rope)       # rows in the epilogue's order
    want_c, want_s = gpu_layout(codes_r, scale_r, rope=bool(rope), swiglu=kw.get("swiglu", False))
    dc, ds = int((Wq.cpu() != want_c).sum()), int((sc.cpu() != want_s).sum())
    print(f"code bytes differing from the reference: {dc}, scale bytes: {ds}")
    assert dc == 0 and ds == 0
    # the dequantise kernel: ref.dequantize_mxfp4 of the natural-order reference, rows in natural order
    nat_c, nat_s = ref.quantize_mxfp4(W.cpu(), gam.cpu())
    back = ops.unshuffle_weight_mxfp4(Wq, sc, **kw)
    assert back.shape == (N, K) and back.dtype == torch.bfloat16
    assert torch.equal(back.cpu().view(torch.int16), ref.dequantize_mxfp4(nat_c, nat_s).view(torch.int16))


def test_quantiser_hand_made_blocks():
    W = hand_blocks()
    Wq, sc = ops.shuffle_weight_mxfp4(W.to(DEV))
    codes_r, scale_r = ref.quantize_mxfp4(W)
    want_c, want_s = gpu_layout(codes_r, scale_r)
    assert torch.equal(Wq.cpu(), want_c) and torch.equal(sc.cpu(), want_s)
    back = ops.unshuffle_weight_mxfp4(Wq, sc).cpu()
    assert torch.equal(back.view(torch.int16), ref.dequantize_mxfp4(codes_r, scale_r).view(torch.int16))
    assert torch.isfinite(back.float()).all()


def rope_setup(M, hkv, d, seed=0):
    g = torch.Generator(device=DEV).manual_seed(100 + seed)
    positions = torch.randint(0, 4000, (M,), device=DEV, dtype=torch.int64, generator=g)
    nb = 8
    slots = torch.randperm(nb * 32, device=DEV, generator=g)[:M].to(torch.int64)
    kc = torch.zeros(nb, hkv, 32, d, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros(nb, hkv, d, 32, dtype=torch.bfloat16, device=DEV)
    return positions, slots, kc, vc


def block_weight(N, K):
    """W[n, k] = 4 * 2^f(n, k // 32), f in 0..7: every code is 6 (the value 4) and block (n, b)'s scale
    byte is 127 + f(n, b), a function of row and block that differs between neighbours either way."""
    n, b = torch.arange(N)[:, None], torch.arange(K // 32)[None, :]
    f = (3 * n + 5 * b) % 8
    W = (4.0 * torch.exp2(f.float())).repeat_interleave(32, dim=1).to(torch.bfloat16)
    return W, f


def block_probe(K):
    """16 activation rows: row m is 1 on the blocks b = m mod 16, 0 elsewhere, so output (m, n) is
    128 * sum over those blocks of 2^f(n, b): exact in fp32 whatever the order of summation."""
    x = torch.zeros(16, K, dtype=torch.bfloat16)
    blk = torch.arange(K) // 32
    x[blk % 16, torch.arange(K)] = 1.0
    return x


def block_sums(f):
    """[16, N] fp32: 128 * sum_{b = m mod 16} 2^f(n, b)."""
    N, B = f.shape
    out = torch.zeros(16, N)
    for b in range(B):
        out[b % 16] += 128.0 * torch.exp2(f[:, b].float())
    return out


@pytest.mark.parametrize("form,N,K", [("plain", 48, 512), ("kmajor", 64, 12288), ("chunked", 65536, 512),
                                      ("swiglu", 192, 1024), ("rope", 512, 512)])
def test_scale_indexing_closed_form(form, N, K):
    """Constant codes and a scale byte that is a known function of (row, block): a scale read from
    another row (gate vs up, a pair partner's, another tile's) or another block of the row changes the
    closed-form output. Tile-major, k-major, the lm_head's k-chunks, SwiGLU's paired chunks and the
    ROPE permutation with its chunks."""
    W, f = block_weight(N, K)
    x = block_probe(K)
    order, C = record_order(N, K, form == "rope", form == "swiglu")
    assert {"plain": order == 0, "kmajor": order == 1, "chunked": order == 5 and C == 4,
            "swiglu": order == 5 and C == 4 and K // 128 > C, "rope": order == 3 and C == 1}[form]
    if form == "rope":
        hq, hkv, d = 2, 1, 128
        assert N == (hq + 2 * hkv) * d
        kw = dict(rope_heads=hq + hkv, head_dim=d)
    else:
        kw = dict(swiglu=True) if form == "swiglu" else {}
    Wq, sc = ops.shuffle_weight_mxfp4(W.to(DEV), **kw)
    perm = ref.rope_row_perm(N, hq + hkv, d) if form == "rope" else torch.arange(N)
    want_c, want_s = gpu_layout(torch.full((N, K // 2), 0x66, dtype=torch.uint8), (127 + f[perm]).to(torch.uint8),
                                rope=form == "rope", swiglu=form == "swiglu")
    assert torch.equal(Wq.cpu(), want_c) and torch.equal(sc.cpu(), want_s)
    sums = block_sums(f)                                        # exact projection, natural row order
    if form == "rope":
        one, zero = torch.ones(64, d // 2), torch.zeros(64, d // 2)
        # cos = 1, sin = 0: every output is its own column; cos = 0, sin = 1: every q/k output is
        # (+-) its pair partner's column
        for cs in (torch.cat([one, zero], 1), torch.cat([zero, one], 1)):
            positions, slots, kc, vc = rope_setup(16, hkv, d)
            positions = positions % 64
            q = ops.skinny_gemm_rope(x.to(DEV), Wq, ops.PRO_PLAIN, positions, cs.to(DEV), kc, vc, slots, hq, hkv, d,
                                     wscale=sc)
            kc_r, vc_r = torch.zeros_like(kc).cpu(), torch.zeros_like(vc).cpu()
            q_r = ref.rope_and_cache(sums, positions.cpu(), cs, kc_r, vc_r, slots.cpu(), hq, hkv, d)
            assert torch.equal(q.float().cpu(), q_r.to(torch.bfloat16).float())
            assert torch.equal(kc.cpu(), kc_r) and torch.equal(vc.cpu(), vc_r)
        return
    if form == "swiglu":
        I = N // 2
        got = ops.skinny_gemm(x.to(DEV), Wq, ops.PRO_PLAIN, ops.EPI_SWIGLU, wscale=sc)
        gate, up = sums[:, :I], sums[:, I:]                     # gate >= 128: silu(gate) = gate in fp32
        assert torch.equal(torch.nn.functional.silu(gate), gate)
        assert torch.equal(got.float().cpu(), (gate * up).to(torch.bfloat16).float())
        return
    got = ops.skinny_gemm(x.to(DEV), Wq, ops.PRO_PLAIN, ops.EPI_STORE, wscale=sc)
    assert torch.equal(got.float().cpu(), sums.to(torch.bfloat16).float())


def gemm_cases(M, N, K):
    """Every required prologue x epilogue at one shape; three calls bit-identical."""
    x = bf(M, K, seed=51)
    W = bf(N, K, scale=0.05, seed=52)
    gam = bf(K, seed=53)
    xc = x.cpu()

    def thrice(fn):
        outs = [fn() for _ in range(3)]
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        return outs[0]

    for pro, g in ((ops.PRO_PLAIN, None), (ops.PRO_NORM, gam)):
        Wq, sc = ops.shuffle_weight_mxfp4(W, g)
        Wd = ops.unshuffle_weight_mxfp4(Wq, sc).cpu()
        got = thrice(lambda: ops.skinny_gemm(x, Wq, pro, wscale=sc))
        close(got, ref.skinny_gemm(xc, Wd, pro).to(DEV), 0.05, 0.02)
        # residual epilogue, in place
        res0 = bf(M, N, seed=54)
        res_ref = res0.cpu().clone()
        ref.skinny_gemm(xc, Wd, pro, 1, res=res_ref)

        def resid():
            r = res0.clone()
            assert ops.skinny_gemm(x, Wq, pro, ops.EPI_RESID, res=r, wscale=sc) is None
            return r
        close(thrice(resid), res_ref.to(DEV), 0.06, 0.02)
        # SwiGLU over [gate; up]: the weights of tests/test_gemm_gpu.py (std 0.05); the oracle's weight
        # is the kernel's exactly, so nothing but summation order and the output rounding differs
        W2 = bf(2 * N, K, scale=0.05, seed=55)
        Wq2, sc2 = ops.shuffle_weight_mxfp4(W2, g, swiglu=True)
        Wd2 = ops.unshuffle_weight_mxfp4(Wq2, sc2, swiglu=True).cpu()
        got = thrice(lambda: ops.skinny_gemm(x, Wq2, pro, ops.EPI_SWIGLU, wscale=sc2))
        close(got, ref.skinny_gemm(xc, Wd2, pro, 2).to(DEV), 0.05, 0.03)


@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("N,K", [(48, 128), (256, 512), (4096, 4096), (1024, 14336), (65536, 512)])
def test_skinny_gemm_mxfp4_modes(M, N, K):
    # record orders (skinny_core.h weight_order): (1024, 14336) k-major, (65536, 512) k-chunks (the
    # lm_head rule: one chunk = all four records), SwiGLU chunks where K allows, the rest tile-major;
    # (48, 128) is 3 tiles of ONE record (three of the four waves idle); K = 512 leaves each wave one record
    gemm_cases(M, N, K)


@pytest.mark.parametrize("M", [20, 32])
def test_skinny_gemm_mxfp4_two_launch_rows(M):
    gemm_cases(M, 4096, 4096)


@pytest.mark.parametrize("M,hq,hkv,d,bias", [(1, 32, 8, 128, False), (3, 32, 8, 128, False), (16, 12, 4, 64, False),
                                              (3, 4, 1, 128, True), (20, 4, 1, 128, True)])
def test_skinny_gemm_rope_mxfp4(M, hq, hkv, d, bias):
    """qkv GEMM on mxfp4 weights + RMSNorm + (Qwen2 bias) + RoPE + paged K/V scatter == the fp32 GEMM
    on the dequantised weight -> K2 reference; tolerances of test_skinny_gemm_rope_epilogue."""
    K = 512
    N = (hq + 2 * hkv) * d
    x = bf(M, K, seed=61)
    W = bf(N, K, scale=0.05, seed=62)
    gam = bf(K, seed=63)
    b = bf(N, scale=0.5, seed=64) if bias else None
    cos_sin = ref.rope_cos_sin(4096, d, 500000.0, DEV)
    positions, slots, kc, vc = rope_setup(M, hkv, d, seed=M)
    kw = dict(rope_heads=hq + hkv, head_dim=d)
    Wq, sc = ops.shuffle_weight_mxfp4(W, gam, **kw)
    qs = []
    for _ in range(3):
        kc.zero_()
        vc.zero_()
        qs.append(ops.skinny_gemm_rope(x, Wq, ops.PRO_NORM, positions, cos_sin, kc, vc, slots, hq, hkv, d, 1e-5,
                                       bias=ops.rope_bias(b, hq, hkv, d) if bias else None, wscale=sc))
    assert torch.equal(qs[0], qs[1]) and torch.equal(qs[0], qs[2])
    Wd = ops.unshuffle_weight_mxfp4(Wq, sc, **kw).cpu()                 # natural row order
    Wp = Wd[ref.rope_row_perm(N, hq + hkv, d)]
    kc_r, vc_r = torch.zeros_like(kc).cpu(), torch.zeros_like(vc).cpu()
    q_r = ref.skinny_gemm_rope(x.cpu(), Wp, 1, positions.cpu(), cos_sin.cpu(), kc_r, vc_r, slots.cpu(), hq, hkv, d,
                               1e-5, bias=ops.rope_bias(b.cpu(), hq, hkv, d) if bias else None)
    close(qs[0], q_r.to(DEV), 0.05, 0.02)
    close(kc, kc_r.to(DEV), 0.05, 0.02)          # chunk-major K blocks, as the reference writes them
    close(vc, vc_r.to(DEV), 0.05, 0.02)


def test_unsupported_forms_raise_on_gpu():
    x = bf(2, 128, seed=1)
    Wq, sc = ops.shuffle_weight_mxfp4(bf(32, 128, scale=0.05, seed=2))
    with pytest.raises(ValueError, match="split"):
        ops.skinny_gemm(x, Wq, wscale=sc, split_ws=ops.split_workspace(DEV))
    with pytest.raises(ValueError, match="x2"):
        ops.skinny_gemm(x, Wq, ops.PRO_NORM_ADD, x2=x, wscale=sc)
    with pytest.raises(ValueError, match="wscale"):
        ops.skinny_gemm(x, Wq)
    with pytest.raises(ValueError, match="K/32"):
        ops.skinny_gemm(x, Wq, wscale=sc[:, :2].contiguous())
    with pytest.raises(ValueError, match="K %"):
        ops.shuffle_weight_mxfp4(bf(32, 192, seed=3))
    # the native entry points check for themselves: a scale array that is not one byte per block
    from theroundtaible_amd.ops import native
    out = torch.empty(2, 32, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="K/32"):
        native().skinny_gemm_mxfp4(out, x, Wq, sc.flatten()[:-1].contiguous(), 0, 0, None, 1e-5)
    with pytest.raises(RuntimeError, match="K/2"):
        native().skinny_gemm_mxfp4(out, x, torch.zeros(32, 128, dtype=torch.uint8, device=DEV), sc, 0, 0, None, 1e-5)
    with pytest.raises(RuntimeError, match="M <= 16"):
        native().skinny_gemm_mxfp4(torch.empty(17, 32, dtype=torch.bfloat16, device=DEV), bf(17, 128), Wq, sc, 0, 0,
                                   None, 1e-5)


def mx_engine(model, **kw):
    from theroundtaible_amd.engine import Engine, EngineConfig
    cfg = dict(model=model, weights="random-full:5", device=DEV, num_blocks=64, weight_quant="mxfp4")
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


@pytest.mark.parametrize("model", ["tiny-llama-128", "tiny-qwen-128"])
def test_mxfp4_fused_decode_matches_unfused(model):
    """Both paths compute with the same dequantised weights, so the bound of
    test_fused_decode_matches_unfused (cosine > 0.999) carries over."""
    from theroundtaible_amd.models.llama import AttnMeta
    e = mx_engine(model, use_graphs=False)
    assert e.weight_residency == "mxfp4" and e.model.quant == "mxfp4"
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
    assert e.model.fused_decode_ok(tok) and not e.model.fused_decode_ok(torch.zeros(33, dtype=torch.long, device=DEV))
    fused = e.model.forward(tok, pos, e.kv, meta).float()
    e.model.use_fused = False
    plain = e.model.forward(tok, pos, e.kv, meta).float()
    cos = torch.nn.functional.cosine_similarity(fused, plain, dim=-1)
    print(f"fused vs unfused cosine min = {float(cos.min())}")
    assert float(cos.min()) > 0.999


@pytest.mark.parametrize("model", ["tiny-llama-128", "tiny-qwen-128"])
def test_mxfp4_engine_graphs_deterministic(model):
    from theroundtaible_amd.engine import SamplingParams, Turn
    sp = SamplingParams(temperature=0.0, max_new_tokens=24, ignore_eos=True, stop_on_consensus=False)
    outs = []
    for _ in range(2):
        e = mx_engine(model)
        assert e.ecfg.use_graphs
        r = e.run_turns([Turn("a", "determinisme met vier bits", sp), Turn("b", "nog een", sp)])
        assert all(t.error is None and len(t.ids) == 24 for t in r)
        outs.append([t.ids for t in r])
    assert outs[0] == outs[1]


@pytest.mark.parametrize("model", ["tiny-llama-128", "tiny-qwen-128"])
def test_mxfp4_prefill_logits_match_cpu(model):
    """HIP-path prefill vs the CPU mxfp4 engine on the same weights: the bound tests/test_fp8_gpu.py
    uses for the same comparison (cosine > 0.99)."""
    from theroundtaible_amd.engine import Engine, EngineConfig
    g = mx_engine(model, use_graphs=False)
    c = Engine(EngineConfig(model=model, weights="random-full:5", device="cpu", dtype="fp32", num_blocks=512,
                            weight_quant="mxfp4"))
    ids = g.encode_prompt("De ridders van de ronde tafel bespreken de architectuur van de cache-laag. " * 3)
    lg = g.prefill([(g.kv.seq("a"), ids)]).float().cpu()
    lc = c.prefill([(c.kv.seq("a"), ids)]).float()
    cos = torch.nn.functional.cosine_similarity(lg, lc, dim=-1)
    print(f"GPU vs CPU mxfp4 prefill cosine min = {float(cos.min())}")
    assert float(cos.min()) > 0.99


def test_mxfp4_refusals_on_gpu():
    from theroundtaible_amd.engine import Engine, EngineConfig
    from theroundtaible_amd.errors import ConfigError
    with pytest.raises(ConfigError, match="'mxfp4' needs dtype bf16"):
        Engine(EngineConfig(model="tiny-llama-128", device=DEV, dtype="fp16", weight_quant="mxfp4"))
    with pytest.raises(ConfigError, match=r"mxfp4 k-record \(128\)"):
        Engine(EngineConfig(model="tiny-llama-128", device=DEV, weight_quant="mxfp4", model_overrides={"ffn": 192}))


def test_mxfp4_load_peak_and_residency():
    """Quantising one linear at a time and freeing its row-major tensor: the load peak does not exceed
    one bf16 weight copy plus the quantised copy; afterwards the linears hold exactly 17/32 byte per
    weight (N K / 2 code bytes + N K / 32 scale bytes)."""
    import gc
    from theroundtaible_amd.engine import Engine, EngineConfig
    gc.collect()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e = Engine(EngineConfig(model="llama3-8b", weights="random:5", device=DEV, weight_quant="mxfp4", defer_kv=True,
                            model_overrides={"n_layers": 4}))
    assert e.weight_residency == "mxfp4" and e.model.shuffled_only
    cfg = e.cfg
    wbytes = cfg.n_params() * 2
    peak = torch.cuda.max_memory_allocated() - base
    dec = e.model.decode_weights()
    names = ("wqkv", "wo", "w_gate_up", "w_down")
    codes = [lw[n] for lw in dec["layers"] for n in names] + [dec["lm_head"]]
    scales = [lw[n + "_scale"] for lw in dec["layers"] for n in names] + [dec["lm_head_scale"]]
    assert all(c.dtype == torch.uint8 for c in codes) and all(s.dtype == torch.uint8 for s in scales)
    assert all(e.model.w[k] is None for k in e.model.w if k.endswith(names) or k == "lm_head")
    h, f, hd = cfg.hidden, cfg.ffn, cfg.head_dim
    per_layer = (cfg.n_heads + 2 * cfg.n_kv_heads) * hd * h + h * cfg.n_heads * hd + 2 * f * h + h * f
    nk = 4 * per_layer + dec["lm_head"].shape[0] * h                     # N K summed over the linears
    resident = sum(t.numel() * t.element_size() for t in codes + scales)
    print(f"load peak {peak / 2**30:.3f} GiB, one bf16 copy {wbytes / 2**30:.3f} GiB, quantised copy "
          f"{resident / 2**30:.3f} GiB")
    assert resident == nk * 17 // 32 and nk % 32 == 0
    assert peak <= wbytes + resident, (peak / 2**30, wbytes / 2**30, resident / 2**30)
    # what stays allocated: the quantised linears + the bf16 embedding / norms (+ the RoPE table)
    other = wbytes - 2 * nk
    now = torch.cuda.memory_allocated() - base
    print(f"resident after load {now / 2**30:.3f} GiB")
    assert now <= resident + other + (256 << 20)
    del e
