"""MXFP4 weight-only quantisation (e2m1 codes + one e8m0 scale byte per 32 k, bf16 activations)
without a GPU: the quantiser contract of ops/reference.py against an independent brute-force
statement of the format, the CPU forms of the new ops, the engine plumbing and the refusals."""
import math

import pytest
import torch

from theroundtaible_amd import ops
from theroundtaible_amd.engine import Engine, EngineConfig, SamplingParams, Turn
from theroundtaible_amd.errors import ConfigError
from theroundtaible_amd.ops import reference as ref

GREEDY = SamplingParams(temperature=0.0, max_new_tokens=8, ignore_eos=True, stop_on_consensus=False)
MAGS = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
BF16_MAX = torch.finfo(torch.bfloat16).max


def brute_force(W, gamma=None):
    """Independent of ref.quantize_mxfp4: python floats (doubles hold every fp32 product, power-of-two
    quotient and distance here exactly), math.frexp for the exponent, nearest of the 16 code values
    by distance with ties to the even code, the sign from copysign. Returns (codes [N, K], e [N, K/32])
    unpacked."""
    N, K = W.shape
    wf = W.double() if gamma is None else (W.float() * gamma.float()[None, :]).double()
    codes = torch.zeros(N, K, dtype=torch.uint8)
    scales = torch.zeros(N, K // 32, dtype=torch.uint8)
    for n in range(N):
        for b in range(K // 32):
            blk = [float(v) for v in wf[n, 32 * b:32 * b + 32]]
            amax = max(abs(v) for v in blk)
            # fp32 exponent field: 0 for zero / fp32 subnormals, else floor(log2 amax) + 127
            E = 0 if amax < 2.0 ** -126 else math.frexp(amax)[1] - 1 + 127
            e = max(E - 2, 2)
            scales[n, b] = e
            for j, v in enumerate(blk):
                y = min(abs(v) / 2.0 ** (e - 127), 6.0)
                best = min(range(8), key=lambda c: (abs(MAGS[c] - y), c & 1))   # ties: the even code
                codes[n, 32 * b + j] = best | (8 if math.copysign(1.0, v) < 0 else 0)
    return codes, scales


def unpack(codes):
    return torch.stack([codes & 15, codes >> 4], dim=2).reshape(codes.shape[0], -1)


def values(codes, scales):
    """Value of every unpacked code under its block's scale byte, in doubles."""
    table = torch.tensor(MAGS + [-m for m in MAGS], dtype=torch.float64)
    two_e = torch.exp2(scales.double() - 127).repeat_interleave(32, dim=1)
    return table[codes.long()] * two_e


def hand_blocks():
    """One block per row: every tie value (both signs), values above 6 x scale, an all-zero block, a
    single non-zero, negative zero, bf16 max, a block of bf16 subnormals."""
    rows = []
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    near = [0.2490234375, 0.251953125, 0.74609375, 0.75390625, 5.03125, 4.96875]
    r = torch.zeros(32)
    r[:7] = torch.tensor(ties)
    r[7:14] = -torch.tensor(ties)
    r[14:20] = torch.tensor(near)
    r[20] = 4.0                                   # amax 5 -> E - 127 = 2 -> scale 1: y = the value itself
    rows.append(r)
    rows.append(r * 2.0 ** -20)                   # the same ties under another scale byte
    r = torch.zeros(32)
    r[0], r[1], r[2], r[3] = 7.5, 6.5, -7.75, 6.0   # amax 7.75 -> scale 1: y > 6 clamps to 6
    rows.append(r)
    rows.append(torch.zeros(32))                  # all zero: e = 2, codes 0
    r = torch.zeros(32)
    r[17] = -0.0437
    rows.append(r)                                # a single non-zero
    r = torch.zeros(32)
    r[3], r[4], r[9] = -0.0, 1.0, -1e-3           # negative zero, and a negative that rounds to zero
    rows.append(r)
    r = torch.zeros(32)
    r[0], r[1], r[2] = BF16_MAX, -BF16_MAX, BF16_MAX / 4
    rows.append(r)
    r = torch.zeros(32)
    r[:4] = torch.tensor([2.0 ** -133, 3 * 2.0 ** -133, -(2.0 ** -130), 2.0 ** -127])   # bf16 subnormals
    rows.append(r)
    W = torch.stack(rows).to(torch.bfloat16)
    W = torch.cat([W, W.flip(0)], dim=1)          # two blocks per row, different neighbours
    return torch.cat([W, W], dim=1).repeat(2, 1).contiguous()   # [16, 128]: a shape the ops take


def test_reference_matches_brute_force_on_random_blocks():
    torch.manual_seed(0)
    W = (torch.randn(16, 256) * 0.05).to(torch.bfloat16)
    W[:, 32:64] *= 2.0 ** -30                     # another exponent range
    W[3, 64:96] *= 2.0 ** 40
    gamma = (1 + 0.1 * torch.randn(256)).to(torch.bfloat16)
    for g in (None, gamma):
        codes, scale = ref.quantize_mxfp4(W, g)
        assert codes.dtype == torch.uint8 and codes.shape == (16, 128)
        assert scale.dtype == torch.uint8 and scale.shape == (16, 8)
        bc, bs = brute_force(W, g)
        assert torch.equal(scale, bs) and torch.equal(unpack(codes), bc)
    # the fold is not rounded to bf16 first: quantising the bf16-folded weight gives other codes
    assert not torch.equal(ref.quantize_mxfp4(ref.fold_gamma(W, gamma))[0], ref.quantize_mxfp4(W, gamma)[0])
    # dequantise: exactly value(code) * 2^(e-127), a bf16 value
    codes, scale = ref.quantize_mxfp4(W, gamma)
    d = ref.dequantize_mxfp4(codes, scale)
    assert d.dtype == torch.bfloat16 and torch.equal(d.double(), values(unpack(codes), scale))


def test_reference_on_hand_made_blocks():
    W = hand_blocks()
    codes, scale = ref.quantize_mxfp4(W)
    bc, bs = brute_force(W)
    c = unpack(codes)
    assert torch.equal(scale, bs) and torch.equal(c, bc)
    # the ties, spelled out (row 0: scale byte 127, y = the value): value -> code
    assert scale[0, 0].item() == 127
    assert c[0, :7].tolist() == [0, 2, 2, 4, 4, 6, 6] and c[0, 7:14].tolist() == [8, 10, 10, 12, 12, 14, 14]
    assert c[0, 14:20].tolist() == [0, 1, 1, 2, 7, 6]
    assert scale[1, 0].item() == 107 and torch.equal(c[1, :32], c[0, :32])
    assert scale[2, 0].item() == 127 and c[2, :4].tolist() == [7, 7, 15, 7]
    assert scale[3, 0].item() == 2 and int(c[3, :32].max()) == 0                  # all-zero block
    assert c[4, 17].item() == 8 + 7 and int((c[4, :32] != 0).sum()) == 1           # single non-zero: y = 5.6 -> 6
    assert c[5, 3].item() == 8 and c[5, 9].item() == 8 and c[5, 0].item() == 0     # -0.0 and a tiny negative: code 8
    assert scale[6, 0].item() == 252 and c[6, :3].tolist() == [7, 15, 4]           # bf16 max: y = 7.97 -> 6 x 2^125
    assert scale[7, 0].item() == 2
    d = ref.dequantize_mxfp4(codes, scale)
    assert torch.isfinite(d.float()).all() and torch.equal(d.double(), values(c, scale))
    assert d[5, 3].item() == 0.0 and math.copysign(1.0, d[5, 3].item()) == -1.0


@pytest.mark.parametrize("kw", [{}, {"rope_heads": 4, "head_dim": 128}, {"swiglu": True}])
def test_round_trip_cpu(kw):
    torch.manual_seed(1)
    W = (torch.randn(6 * 128, 256) * 0.05).to(torch.bfloat16)
    gamma = (1 + 0.1 * torch.randn(256)).to(torch.bfloat16)
    Wq, scale = ops.shuffle_weight_mxfp4(W, gamma, **kw)
    assert Wq.dtype == torch.uint8 and Wq.shape == (768, 128) and scale.dtype == torch.uint8 and scale.shape == (768, 8)
    back = ops.unshuffle_weight_mxfp4(Wq, scale, **kw)
    codes, s = ref.quantize_mxfp4(W, gamma)                     # natural row order
    assert back.dtype == torch.bfloat16 and back.shape == W.shape
    assert torch.equal(back, ref.dequantize_mxfp4(codes, s))
    assert torch.equal(back.double(), values(unpack(codes), s))
    if kw.get("rope_heads"):   # the stored rows (and scale bytes) are in the ROPE epilogue's order
        perm = ref.rope_row_perm(W.shape[0], 4, 128)
        assert torch.equal(Wq, codes[perm]) and torch.equal(scale, s[perm]) and not torch.equal(Wq, codes)
    else:
        assert torch.equal(Wq, codes) and torch.equal(scale, s)


def test_skinny_gemm_cpu_runs_the_oracle_on_the_dequantised_weight():
    torch.manual_seed(2)
    W = (torch.randn(64, 128) * 0.05).to(torch.bfloat16)
    x = torch.randn(3, 128).to(torch.bfloat16)
    Wq, scale = ops.shuffle_weight_mxfp4(W)
    y = ops.skinny_gemm(x, Wq, ops.PRO_NORM, ops.EPI_STORE, wscale=scale)
    assert torch.equal(y, ref.skinny_gemm(x, ref.dequantize_mxfp4(Wq, scale), 1, 0))
    # the GEMM error cap: W = N(0, 0.05^2) of shape (64, 128), 3 rows, seed 2; the reference measures
    # 0.125 here, a wrong nibble order or a scale one exponent off gives more than 0.5
    exact = ref.skinny_gemm(x, W, 1, 0).float()
    rel = ((y.float() - exact).norm() / exact.norm()).item()
    print(f"relative GEMM error = {rel}")
    assert rel < 0.2
    swapped = ((Wq & 15) << 4) | (Wq >> 4)
    for bad in (ref.dequantize_mxfp4(swapped, scale), ref.dequantize_mxfp4(Wq, scale + 1)):
        r = ((ref.skinny_gemm(x, bad, 1, 0).float() - exact).norm() / exact.norm()).item()
        assert r > 0.5, r
    # the ROPE form dispatches the same way
    hq, hkv, d = 2, 1, 32
    Wr = (torch.randn((hq + 2 * hkv) * d, 128) * 0.05).to(torch.bfloat16)
    Wq2, s2 = ops.shuffle_weight_mxfp4(Wr, rope_heads=hq + hkv, head_dim=d)
    cs = ref.rope_cos_sin(64, d, 10000.0, "cpu")
    pos, slots = torch.tensor([1, 5, 9]), torch.tensor([0, 33, 70])
    kc = [torch.zeros(4, hkv, 32, d, dtype=torch.bfloat16) for _ in range(2)]
    vc = [torch.zeros(4, hkv, d, 32, dtype=torch.bfloat16) for _ in range(2)]
    q = ops.skinny_gemm_rope(x, Wq2, ops.PRO_NORM, pos, cs, kc[0], vc[0], slots, hq, hkv, d, wscale=s2)
    q_r = ref.skinny_gemm_rope(x, ref.dequantize_mxfp4(Wq2, s2), 1, pos, cs, kc[1], vc[1], slots, hq, hkv, d)
    assert torch.equal(q, q_r) and torch.equal(kc[0], kc[1]) and torch.equal(vc[0], vc[1])


def test_unsupported_forms_raise():
    W = (torch.randn(32, 128) * 0.05).to(torch.bfloat16)
    x = torch.randn(2, 128).to(torch.bfloat16)
    Wq, scale = ops.shuffle_weight_mxfp4(W)
    with pytest.raises(ValueError, match="x2"):
        ops.skinny_gemm(x, Wq, ops.PRO_NORM_ADD, ops.EPI_STORE, x2=x, wscale=scale)
    with pytest.raises(ValueError, match="x2"):
        ops.skinny_gemm(x, Wq, xout=torch.empty_like(x), wscale=scale)
    with pytest.raises(ValueError, match="split"):
        ops.skinny_gemm(x, Wq, wscale=scale, split_ws=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="rows"):
        ops.skinny_gemm(torch.zeros(33, 128, dtype=torch.bfloat16), Wq, wscale=scale)
    with pytest.raises(ValueError, match="wscale"):
        ops.skinny_gemm(x, Wq)                       # codes without scales: never a silent bf16 read
    with pytest.raises(ValueError, match="uint8"):
        ops.skinny_gemm(x, W, wscale=scale)          # scale bytes without uint8 codes
    with pytest.raises(ValueError, match="K %"):
        ops.skinny_gemm(torch.zeros(2, 192, dtype=torch.bfloat16), torch.zeros(32, 96, dtype=torch.uint8),
                        wscale=torch.zeros(32, 6, dtype=torch.uint8))
    with pytest.raises(ValueError, match="K/32"):
        ops.skinny_gemm(x, Wq, wscale=scale[:, :2])  # a scale array of another weight
    with pytest.raises(ValueError, match="K %"):
        ops.shuffle_weight_mxfp4(torch.zeros(16, 192, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="N %"):
        ops.shuffle_weight_mxfp4(torch.zeros(24, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="split"):
        ops.skinny_gemm_rope(x, Wq, ops.PRO_NORM, None, None, None, None, None, 1, 0, 32, wscale=scale,
                             split_ws=torch.zeros(4, dtype=torch.int32))
    assert ops.MXFP4_K_RECORD == 128


def mx_engine(model, **kw):
    cfg = dict(model=model, device="cpu", dtype="fp32", num_blocks=64, weights="random-full:5", weight_quant="mxfp4")
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


@pytest.mark.parametrize("model", ["tiny-llama-128", "tiny-qwen-128"])
def test_engine_mxfp4_cpu_greedy_turn(model):
    a, b = mx_engine(model), mx_engine(model)
    assert a.weight_residency == "mxfp4" and a.weight_quant == "mxfp4" and a.model.quant == "mxfp4"
    # single copy: the row-major linears are gone, codes and scales are uint8, the embedding is not quantised
    assert a.model.layers[0]["wqkv"] is None and a.model.w["lm_head"] is None and a.model.shuffled_only
    d = a.model.decode_weights()
    for w, s in ((d["layers"][0]["wqkv"], d["layers"][0]["wqkv_scale"]), (d["lm_head"], d["lm_head_scale"]),
                 (d["layers"][-1]["w_down"], d["layers"][-1]["w_down_scale"])):
        assert w.dtype == torch.uint8 and s.dtype == torch.uint8 and s.shape == (w.shape[0], w.shape[1] // 16)
    plain = Engine(EngineConfig(model=model, device="cpu", dtype="fp32", num_blocks=64, weights="random-full:5"))
    assert plain.weight_quant == "none"
    assert a.model.w["embed"].dtype == a.dtype and torch.equal(a.model.w["embed"], plain.model.w["embed"])
    ta = a.run_turns([Turn("K", "Een ronde tafel met vier-bits gewichten.", GREEDY)])[0]
    tb = b.run_turns([Turn("K", "Een ronde tafel met vier-bits gewichten.", GREEDY)])[0]
    assert ta.error is None and len(ta.ids) == GREEDY.max_new_tokens
    assert ta.ids == tb.ids
    # the engine computes with the dequantised weights: logits differ from the bf16-weight engine's
    ids = a.encode_prompt("Een gedeelde sleutel voor de ronde tafel, graag. " * 2)
    la = a.prefill([(a.kv.seq("p"), ids)]).float()
    lr = plain.prefill([(plain.kv.seq("p"), ids)]).float()
    cos = torch.nn.functional.cosine_similarity(la.flatten(), lr.flatten(), dim=0).item()
    print(f"mxfp4 vs bf16 prefill logits cosine = {cos}")
    assert torch.isfinite(la).all() and not torch.equal(la, lr) and cos < 1.0


def test_env_default_and_explicit_none(monkeypatch):
    monkeypatch.setenv("ROUNDTABLE_WEIGHT_QUANT", "mxfp4")
    assert EngineConfig(model="tiny-llama-128").weight_quant == "mxfp4"
    assert EngineConfig(model="tiny-llama-128", weight_quant="none").weight_quant == "none"
    assert EngineConfig(model="tiny-llama-128", weight_quant="fp8").weight_quant == "fp8"
    monkeypatch.delenv("ROUNDTABLE_WEIGHT_QUANT")
    assert EngineConfig(model="tiny-llama-128").weight_quant == "none"
    with pytest.raises(ConfigError):
        Engine(EngineConfig(model="tiny-llama-128", device="cpu", weight_quant="int4"))


def test_serve_weight_quant_parses():
    from theroundtaible_amd.cli import build_parser
    p = build_parser()
    assert p.parse_args(["serve", "--weight-quant", "mxfp4"]).weight_quant == "mxfp4"
    assert p.parse_args(["serve", "--weight-quant", "fp8"]).weight_quant == "fp8"
    with pytest.raises(SystemExit):
        p.parse_args(["serve", "--weight-quant", "int4"])


def _config(quants):
    from theroundtaible_amd.types import RoundtableConfig
    knights = [{"name": f"Ridder{i}", "adapter": f"local-llm-r{i}", "capabilities": ["x"], "priority": i + 1}
               for i in range(len(quants))]
    return RoundtableConfig.from_dict({
        "version": "1.0", "project": "mxfp4", "language": "nl", "knights": knights,
        "rules": {"max_rounds": 1, "consensus_threshold": 9, "timeout_per_turn_seconds": 300,
                  "escalate_to_user_after": 5, "auto_execute": False, "ignore": [".git"], "round_mode": "parallel"},
        "chronicle": ".roundtable/chronicle.md",
        "engine": {"default_model": "tiny-llama-128", "max_new_tokens": 4, "ignore_eos": True, "temperature": 0.0,
                   "device": "cpu", "weights": "random-full:3"},
        "adapter_config": {f"local-llm-r{i}": {"engine": ({"weight_quant": q} if q else {})}
                           for i, q in enumerate(quants)}})


def test_config_plumbing_and_pool_keys(monkeypatch):
    from theroundtaible_amd.config import WEIGHT_QUANTS, engine_settings
    from theroundtaible_amd.knights.registry import BackendFactory
    monkeypatch.delenv("ROUNDTABLE_WEIGHT_QUANT", raising=False)
    assert WEIGHT_QUANTS == ("none", "fp8", "mxfp4")
    quants = ["mxfp4", None, "fp8", "mxfp4"]
    cfg = _config(quants)
    got = [engine_settings(cfg, f"local-llm-r{i}")["weight_quant"] for i in range(4)]
    assert got == ["mxfp4", "none", "fp8", "mxfp4"]
    factory = BackendFactory(cfg)
    b = [factory.create(f"local-llm-r{i}") for i in range(4)]
    assert [x.engine.ecfg.weight_quant for x in b] == got
    # three quant values of one model: three engines, the two mxfp4 knights share theirs
    assert b[0].engine is b[3].engine and len({id(x.engine) for x in b}) == 3 and len(factory.pool.engines) == 3
    assert [x.engine.weight_residency for x in b[:3]][0] == "mxfp4" and b[2].engine.weight_residency == "fp8"
    assert b[1].engine.weight_residency not in ("fp8", "mxfp4")
    # an engine-wide setting applies to every knight; the environment only fills what is unstated
    cfg2 = _config([None, "none"])
    cfg2.raw["engine"]["weight_quant"] = "mxfp4"
    assert [engine_settings(cfg2, f"local-llm-r{i}")["weight_quant"] for i in range(2)] == ["mxfp4", "none"]
    monkeypatch.setenv("ROUNDTABLE_WEIGHT_QUANT", "mxfp4")
    cfg3 = _config([None, "none", "fp8"])
    assert [engine_settings(cfg3, f"local-llm-r{i}")["weight_quant"] for i in range(3)] == ["mxfp4", "none", "fp8"]
    for unknown in ("int4", "int3"):
        with pytest.raises(ConfigError):
            engine_settings(_config([unknown]), "local-llm-r0")


def test_refusals():
    from theroundtaible_amd.parallel.tp import TPInfo
    with pytest.raises(ConfigError, match="'mxfp4' does not support tensor parallel"):
        Engine(EngineConfig(model="tiny-llama-128", device="cpu", weight_quant="mxfp4"), TPInfo(size=2, rank=0))
    with pytest.raises(ConfigError, match="'mxfp4' needs a model family"):
        Engine(EngineConfig(model="tiny-gpt2", device="cpu", weight_quant="mxfp4"))
    # GEMM depths the 128-deep record does not divide: ffn 96, and ffn 192 — a multiple of 64, which fp8 takes
    for ffn in (96, 192):
        with pytest.raises(ConfigError, match=r"'mxfp4': ffn / tp = %d is not a multiple of the mxfp4 k-record \(128\)" % ffn):
            Engine(EngineConfig(model="tiny-llama-128", device="cpu", weight_quant="mxfp4", model_overrides={"ffn": ffn}))
    e = Engine(EngineConfig(model="tiny-llama-128", device="cpu", weight_quant="fp8", model_overrides={"ffn": 192}))
    assert e.weight_residency == "fp8"
