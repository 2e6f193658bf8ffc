"""FP8 weight-only decode GEMMs on the GPU (csrc/gemm_skinny_fp8.hip): quantiser, every prologue x
epilogue of the fp8 launch, scale indexing, the RoPE epilogue, the engine paths and residency.

The GEMM oracle is ref.skinny_gemm / ref.skinny_gemm_rope on the weight ``unshuffle_weight_fp8``
rebuilds from the GPU's own codes, so the GEMM tests do not depend on quantiser tie-breaking; the
tolerances are those tests/test_gemm_gpu.py uses for the same epilogues."""
import pytest
import torch

from theroundtaible_amd import ops
from theroundtaible_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"


def bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(torch.bfloat16)


def close(a, b, atol, rtol=0.0):
    d = (a.float() - b.float()).abs()
    tol = atol + rtol * b.float().abs()
    assert bool((d <= tol).all()), f"max err {d.max().item():.4g}"


def code_values(Wq, scale, **kw):
    """Exact e4m3 values of the GPU's codes, natural row order: dequantise with unit scales."""
    return ops.unshuffle_weight_fp8(Wq, torch.ones_like(scale), **kw).float().cpu()


def half_spacing(y):
    e = torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -20)))
    return 0.5 * torch.maximum(torch.exp2(e - 3), torch.tensor(2.0 ** -9))


@pytest.mark.parametrize("N,K,kw", [(48, 128, {}), (256, 512, {}), (1024, 14336, {}),
                                    (6 * 128, 256, {"rope_heads": 4, "head_dim": 128}),
                                    (512, 4096, {"swiglu": True})])
def test_quantiser(N, K, kw):
    W = bf(N, K, scale=0.05, seed=11)
    gam = bf(K, seed=12)
    Wq, scale = ops.shuffle_weight_fp8(W, gam, **kw)
    assert Wq.dtype == torch.uint8 and Wq.shape == (N, K) and scale.dtype == torch.float32
    v = code_values(Wq, scale, **kw)
    wf = W.float().cpu() * gam.float().cpu()[None, :]
    amax = wf.abs().amax(dim=1)
    y = wf * (torch.full_like(amax, 448.0) / amax)[:, None]     # one correctly rounded division
    # +-448 at every row's largest element, every code within half a step of its target
    assert torch.equal(v.gather(1, wf.abs().argmax(dim=1)[:, None]).abs().squeeze(1), torch.full_like(amax, 448.0))
    ratio = ((y - v).abs() / half_spacing(y)).max().item()
    print(f"worst |y - code| / half spacing = {ratio}")
    assert ratio <= 1.0, ratio
    # against the reference quantiser: equal except at rounding ties, and then adjacent
    rope = {k: kw[k] for k in ("rope_heads", "head_dim") if k in kw}
    codes_r, _ = ref.quantize_fp8(W.cpu(), gam.cpu())
    _, scale_r = ref.quantize_fp8(W.cpu(), gam.cpu(), **rope)          # scales in the epilogue's row order
    assert torch.allclose(scale.cpu(), scale_r, rtol=1e-6, atol=0)
    got = v.to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(got.view(torch.float8_e4m3fn).float(), v)          # the values ARE e4m3
    diff = got != codes_r
    share = diff.float().mean().item()
    print(f"codes differing from the reference: {share:.3g}")
    assert share <= 1e-4, share
    assert bool(((got[diff].int() - codes_r[diff].int()).abs() == 1).all())
    # the dequantised weight is bf16(code * scale), rows in natural order
    nat_scale = torch.empty(N)
    nat_scale[ref.rope_row_perm(N, rope.get("rope_heads", 0), rope.get("head_dim", 0))] = scale.cpu()
    assert torch.equal(ops.unshuffle_weight_fp8(Wq, scale, **kw).cpu(), (v * nat_scale[:, None]).to(torch.bfloat16))


def test_quantiser_zero_row_and_bf16_max():
    W = bf(32, 128, scale=0.05, seed=13)
    W[3] = 0
    W[5, 7] = torch.finfo(torch.bfloat16).max
    Wq, scale = ops.shuffle_weight_fp8(W)
    v = code_values(Wq, scale)
    assert scale[3].item() == 1.0 and float(v[3].abs().max()) == 0.0
    assert not torch.isnan(v).any() and v[5, 7].item() == 448.0 and torch.isfinite(scale).all()


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
        Wq, sc = ops.shuffle_weight_fp8(W, g)
        Wd = ops.unshuffle_weight_fp8(Wq, sc).cpu()
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
        # SwiGLU over [gate; up]. Weights of std 1 / sqrt(K) (pre-activations of std ~1, as a
        # trained layer's): the oracle's weights are bf16(code * scale), each up to 2^-9 off the
        # code * scale the kernel computes with, so gate and up differ from the oracle's by
        # ~1e-3 of their std, and silu(gate) * up by |gate| times that where up ~ 0. At std 0.05
        # and K = 14336 (gate, up ~ N(0, 6)) that oracle rounding alone reaches 0.1-0.2, past the
        # 0.05 the bound allows at outputs near zero; at unit std it stays below 0.01.
        W2 = bf(2 * N, K, scale=K ** -0.5, seed=55)
        Wq2, sc2 = ops.shuffle_weight_fp8(W2, g, swiglu=True)
        Wd2 = ops.unshuffle_weight_fp8(Wq2, sc2, swiglu=True).cpu()
        got = thrice(lambda: ops.skinny_gemm(x, Wq2, pro, ops.EPI_SWIGLU, wscale=sc2))
        close(got, ref.skinny_gemm(xc, Wd2, pro, 2).to(DEV), 0.05, 0.03)


@pytest.mark.parametrize("M", [1, 3, 16])
@pytest.mark.parametrize("N,K", [(48, 128), (256, 512), (4096, 4096), (1024, 14336), (65536, 512)])
def test_skinny_gemm_fp8_modes(M, N, K):
    # record orders (skinny_core.h weight_order): (1024, 14336) k-major, (65536, 512) k-chunks (the
    # lm_head rule), SwiGLU chunks where K allows, the rest tile-major; (48, 128) is 3 tiles of 2
    # records; K = 512 leaves each wave a single record
    gemm_cases(M, N, K)


@pytest.mark.parametrize("M", [20, 32])
def test_skinny_gemm_fp8_two_launch_rows(M):
    gemm_cases(M, 4096, 4096)


def rope_setup(M, hkv, d, seed=0):
    g = torch.Generator(device=DEV).manual_seed(100 + seed)
    positions = torch.randint(0, 4000, (M,), device=DEV, dtype=torch.int64, generator=g)
    nb = 8
    slots = torch.randperm(nb * 32, device=DEV, generator=g)[:M].to(torch.int64)
    kc = torch.zeros(nb, hkv, 32, d, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros(nb, hkv, d, 32, dtype=torch.bfloat16, device=DEV)
    return positions, slots, kc, vc


@pytest.mark.parametrize("swiglu", [True, False])
def test_scale_indexing_closed_form(swiglu):
    """Weight row n is the constant 2^(n mod 5): every code is 448 and scale[n] = 2^(n mod 5) / 448,
    so with all-ones activations column sums are K * 2^(n mod 5) exactly and any scale read from the
    wrong row (gate vs up, a pair partner's) is off by a power of two."""
    K, M = 64, 3
    x = torch.ones(M, K, dtype=torch.bfloat16, device=DEV)
    if swiglu:
        I = 48                                   # I mod 5 = 3: the gate and up rows' scales differ
        n = torch.arange(2 * I, device=DEV)
        W = torch.exp2((n % 5).float())[:, None].expand(2 * I, K).contiguous().to(torch.bfloat16)
        Wq, sc = ops.shuffle_weight_fp8(W, swiglu=True)
        assert torch.equal(sc, torch.exp2((n % 5).float()) / 448.0)
        got = ops.skinny_gemm(x, Wq, ops.PRO_PLAIN, ops.EPI_SWIGLU, wscale=sc).float()
        gate, up = K * torch.exp2((n[:I] % 5).float()), K * torch.exp2(((n[:I] + I) % 5).float())
        exp = (torch.nn.functional.silu(gate) * up).to(torch.bfloat16).float()
        assert torch.equal(got, exp[None, :].expand(M, I))
        return
    hq, hkv, d = 2, 1, 128                       # D / 2 = 64, 64 mod 5 = 4: pair partners differ
    N = (hq + 2 * hkv) * d
    n = torch.arange(N, device=DEV)
    W = torch.exp2((n % 5).float())[:, None].expand(N, K).contiguous().to(torch.bfloat16)
    Wq, sc = ops.shuffle_weight_fp8(W, rope_heads=hq + hkv, head_dim=d)
    qkv = (K * torch.exp2((n % 5).float()))[None, :].expand(M, N).contiguous().cpu()   # exact projection
    one, zero = torch.ones(64, d // 2), torch.zeros(64, d // 2)
    # cos = 1, sin = 0: every output is its own column; cos = 0, sin = 1: every q/k output is
    # (+-) its pair partner's column, so the partner's scale is checked too
    for cs in (torch.cat([one, zero], 1), torch.cat([zero, one], 1)):
        positions, slots, kc, vc = rope_setup(M, hkv, d)
        positions = positions % 64
        q = ops.skinny_gemm_rope(x, Wq, ops.PRO_PLAIN, positions, cs.to(DEV), kc, vc, slots, hq, hkv, d, wscale=sc)
        kc_r, vc_r = torch.zeros_like(kc).cpu(), torch.zeros_like(vc).cpu()
        q_r = ref.rope_and_cache(qkv, positions.cpu(), cs, kc_r, vc_r, slots.cpu(), hq, hkv, d)
        assert torch.equal(q.float().cpu(), q_r.to(torch.bfloat16).float())
        assert torch.equal(kc.cpu(), kc_r) and torch.equal(vc.cpu(), vc_r)


@pytest.mark.parametrize("M,hq,hkv,d,bias", [(1, 32, 8, 128, False), (3, 32, 8, 128, False), (16, 12, 4, 64, False),
                                              (3, 4, 1, 128, True), (20, 4, 1, 128, True)])
def test_skinny_gemm_rope_fp8(M, hq, hkv, d, bias):
    """qkv GEMM on fp8 weights + RMSNorm + (Qwen2 bias) + RoPE + paged K/V scatter == the fp32 GEMM
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
    Wq, sc = ops.shuffle_weight_fp8(W, gam, **kw)
    qs = []
    for _ in range(3):
        kc.zero_()
        vc.zero_()
        qs.append(ops.skinny_gemm_rope(x, Wq, ops.PRO_NORM, positions, cos_sin, kc, vc, slots, hq, hkv, d, 1e-5,
                                       bias=ops.rope_bias(b, hq, hkv, d) if bias else None, wscale=sc))
    assert torch.equal(qs[0], qs[1]) and torch.equal(qs[0], qs[2])
    Wd = ops.unshuffle_weight_fp8(Wq, sc, **kw).cpu()                   # natural row order
    Wp = Wd[ref.rope_row_perm(N, hq + hkv, d)]
    kc_r, vc_r = torch.zeros_like(kc).cpu(), torch.zeros_like(vc).cpu()
    q_r = ref.skinny_gemm_rope(x.cpu(), Wp, 1, positions.cpu(), cos_sin.cpu(), kc_r, vc_r, slots.cpu(), hq, hkv, d,
                               1e-5, bias=ops.rope_bias(b.cpu(), hq, hkv, d) if bias else None)
    close(qs[0], q_r.to(DEV), 0.05, 0.02)
    close(kc, kc_r.to(DEV), 0.05, 0.02)          # chunk-major K blocks, as the reference writes them
    close(vc, vc_r.to(DEV), 0.05, 0.02)


def test_unsupported_forms_raise_on_gpu():
    x = bf(2, 128, seed=1)
    Wq, sc = ops.shuffle_weight_fp8(bf(32, 128, scale=0.05, seed=2))
    with pytest.raises(ValueError):
        ops.skinny_gemm(x, Wq, wscale=sc, split_ws=ops.split_workspace(DEV))
    with pytest.raises(ValueError):
        ops.skinny_gemm(x, Wq, ops.PRO_NORM_ADD, x2=x, wscale=sc)
    with pytest.raises(ValueError):
        ops.skinny_gemm(x, Wq)


def fp8_engine(model, **kw):
    from theroundtaible_amd.engine import Engine, EngineConfig
    cfg = dict(model=model, weights="random-full:5", device=DEV, num_blocks=64, weight_quant="fp8")
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


@pytest.mark.parametrize("model", ["tiny-llama-128", "tiny-qwen-128"])
def test_fp8_fused_decode_matches_unfused(model):
    """Both paths compute with the same dequantised weights, so the bound of
    test_fused_decode_matches_unfused (cosine > 0.999) carries over."""
    from theroundtaible_amd.models.llama import AttnMeta
    e = fp8_engine(model, use_graphs=False)
    assert e.weight_residency == "fp8" and e.model.quant == "fp8"
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
def test_fp8_engine_graphs_deterministic(model):
    from theroundtaible_amd.engine import SamplingParams, Turn
    sp = SamplingParams(temperature=0.0, max_new_tokens=24, ignore_eos=True, stop_on_consensus=False)
    outs = []
    for _ in range(2):
        e = fp8_engine(model)
        assert e.ecfg.use_graphs
        r = e.run_turns([Turn("a", "determinisme met acht bits", sp), Turn("b", "nog een", sp)])
        assert all(t.error is None and len(t.ids) == 24 for t in r)
        outs.append([t.ids for t in r])
    assert outs[0] == outs[1]


@pytest.mark.parametrize("model", ["tiny-llama-128", "tiny-qwen-128"])
def test_fp8_prefill_logits_match_cpu(model):
    """HIP-path prefill vs the CPU fp8 engine on the same weights: the bound of
    tests/test_engine_gpu.py test_prefill_logits_match_cpu (cosine > 0.99)."""
    from theroundtaible_amd.engine import Engine, EngineConfig
    g = fp8_engine(model, use_graphs=False)
    c = Engine(EngineConfig(model=model, weights="random-full:5", device="cpu", dtype="fp32", num_blocks=512,
                            weight_quant="fp8"))
    ids = g.encode_prompt("De ridders van de ronde tafel bespreken de architectuur van de cache-laag. " * 3)
    lg = g.prefill([(g.kv.seq("a"), ids)]).float().cpu()
    lc = c.prefill([(c.kv.seq("a"), ids)]).float()
    cos = torch.nn.functional.cosine_similarity(lg, lc, dim=-1)
    print(f"GPU vs CPU fp8 prefill cosine min = {float(cos.min())}")
    assert float(cos.min()) > 0.99


def test_fp8_refusals_on_gpu():
    from theroundtaible_amd.engine import Engine, EngineConfig
    from theroundtaible_amd.errors import ConfigError
    with pytest.raises(ConfigError, match="bf16"):
        Engine(EngineConfig(model="tiny-llama-128", device=DEV, dtype="fp16", weight_quant="fp8"))


def test_fp8_load_peak_and_residency():
    """Quantising one linear at a time and freeing its row-major tensor keeps the load peak at one
    bf16 weight copy + one tensor (the bound of test_shuffled_only_load_peak_is_one_weight_copy);
    afterwards the linears hold half their bf16 bytes plus the row scales."""
    import gc
    from theroundtaible_amd.engine import Engine, EngineConfig
    gc.collect()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e = Engine(EngineConfig(model="llama3-8b", weights="random:5", device=DEV, weight_quant="fp8", defer_kv=True,
                            model_overrides={"n_layers": 4}))
    assert e.weight_residency == "fp8" and e.model.shuffled_only
    cfg = e.cfg
    wbytes = cfg.n_params() * 2
    biggest = cfg.vocab * cfg.hidden * 2
    peak = torch.cuda.max_memory_allocated() - base
    print(f"load peak {peak / 2**30:.3f} GiB, one bf16 copy {wbytes / 2**30:.3f} GiB")
    assert peak <= wbytes + 1.05 * biggest + (256 << 20), (peak / 2**30, wbytes / 2**30)
    dec = e.model.decode_weights()
    names = ("wqkv", "wo", "w_gate_up", "w_down")
    codes = [lw[n] for lw in dec["layers"] for n in names] + [dec["lm_head"]]
    scales = [lw[n + "_scale"] for lw in dec["layers"] for n in names] + [dec["lm_head_scale"]]
    assert all(c.dtype == torch.uint8 for c in codes) and all(s.dtype == torch.float32 for s in scales)
    assert all(e.model.w[k] is None for k in e.model.w if k.endswith(names) or k == "lm_head")
    lin_bf16 = sum(c.numel() for c in codes) * 2
    resident = sum(c.numel() * c.element_size() for c in codes)
    scale_bytes = sum(s.numel() * 4 for s in scales)
    assert resident <= 0.5 * lin_bf16
    # what stays allocated: the codes + scales + the bf16 embedding / norms (+ the RoPE table)
    other = wbytes - lin_bf16
    now = torch.cuda.memory_allocated() - base
    print(f"resident after load {now / 2**30:.3f} GiB (linears {resident / 2**30:.3f} + scales {scale_bytes / 2**20:.2f} MiB)")
    assert now <= 0.5 * lin_bf16 + scale_bytes + other + (256 << 20)
    del e
