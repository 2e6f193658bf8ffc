"""FP8 weight-only quantisation (e4m3fn weights, bf16 activations) without a GPU: the quantiser
contract of ops/reference.py, the CPU forms of the new ops, the engine plumbing and the refusals."""
import math

import pytest
import torch

from theroundtaible_amd import ops
from theroundtaible_amd.engine import Engine, EngineConfig, SamplingParams, Turn
from theroundtaible_amd.errors import ConfigError
from theroundtaible_amd.ops import reference as ref

GREEDY = SamplingParams(temperature=0.0, max_new_tokens=8, ignore_eos=True, stop_on_consensus=False)


def fp8_values(codes: torch.Tensor) -> torch.Tensor:
    return codes.view(torch.float8_e4m3fn).float()


def half_spacing(y: torch.Tensor) -> torch.Tensor:
    """Half the e4m3 spacing at |y|: 2^(floor(log2|y|) - 3), floored at the subnormal spacing 2^-9."""
    e = torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -20)))
    return 0.5 * torch.maximum(torch.exp2(e - 3), torch.tensor(2.0 ** -9))


def check_contract(W, gamma, codes, scale):
    """Shared with the GPU test: +-448 at every row's largest element, rounding within half a step."""
    wf = W.float() * gamma.float()[None, :] if gamma is not None else W.float()
    amax = wf.abs().amax(dim=1)
    y = wf * (torch.full_like(amax, 448.0) / amax)[:, None]     # one correctly rounded division
    v = fp8_values(codes)
    assert not torch.isnan(v).any()
    top = wf.abs().argmax(dim=1)
    assert torch.equal(v.gather(1, top[:, None]).abs().squeeze(1), torch.full_like(amax, 448.0))
    ratio = ((y - v).abs() / half_spacing(y)).max().item()
    assert ratio <= 1.0, ratio
    assert torch.allclose(scale, amax / 448.0, rtol=1e-6, atol=0)


def test_quantiser_contract():
    torch.manual_seed(0)
    W = (torch.randn(64, 512) * 0.05).to(torch.bfloat16)
    gamma = (1 + 0.1 * torch.randn(512)).to(torch.bfloat16)
    codes, scale = ref.quantize_fp8(W, gamma)
    assert codes.dtype == torch.uint8 and codes.shape == W.shape and scale.dtype == torch.float32
    check_contract(W, gamma, codes, scale)
    # the fold is not rounded to bf16 first: quantising the bf16-folded weight gives other codes
    folded = ref.fold_gamma(W, gamma)
    assert not torch.equal(ref.quantize_fp8(folded)[0], codes)


def test_quantiser_zero_row_and_bf16_max():
    W = (torch.randn(16, 64) * 0.05).to(torch.bfloat16)
    W[3] = 0
    W[5, 7] = torch.finfo(torch.bfloat16).max
    W[6, 1] = -torch.finfo(torch.bfloat16).max
    codes, scale = ref.quantize_fp8(W)
    assert scale[3].item() == 1.0 and int(codes[3].max()) == 0
    v = fp8_values(codes)
    assert not torch.isnan(v).any() and torch.isfinite(scale).all()
    assert v[5, 7].item() == 448.0 and v[6, 1].item() == -448.0
    assert not torch.isnan(ref.dequantize_fp8(codes, scale).float()).any()


@pytest.mark.parametrize("kw", [{}, {"rope_heads": 4, "head_dim": 128}, {"swiglu": True}])
def test_round_trip_cpu(kw):
    torch.manual_seed(1)
    W = (torch.randn(6 * 128, 256) * 0.05).to(torch.bfloat16)
    gamma = (1 + 0.1 * torch.randn(256)).to(torch.bfloat16)
    Wq, scale = ops.shuffle_weight_fp8(W, gamma, **kw)
    assert Wq.dtype == torch.uint8 and Wq.shape == W.shape and scale.shape == (W.shape[0],)
    back = ops.unshuffle_weight_fp8(Wq, scale, **kw)
    codes, s = ref.quantize_fp8(W, gamma)                       # natural row order
    assert back.dtype == torch.bfloat16
    assert torch.equal(back, ref.dequantize_fp8(codes, s))
    assert torch.equal(back, (fp8_values(codes) * s[:, None]).to(torch.bfloat16))
    if kw.get("rope_heads"):   # the stored rows (and scales) are in the ROPE epilogue's order
        perm = ref.rope_row_perm(W.shape[0], 4, 128)
        assert torch.equal(Wq, codes[perm]) and torch.equal(scale, s[perm])


def test_skinny_gemm_cpu_runs_the_oracle_on_the_dequantised_weight():
    torch.manual_seed(2)
    W = (torch.randn(64, 128) * 0.05).to(torch.bfloat16)
    x = torch.randn(3, 128).to(torch.bfloat16)
    Wq, scale = ops.shuffle_weight_fp8(W)
    y = ops.skinny_gemm(x, Wq, ops.PRO_NORM, ops.EPI_STORE, wscale=scale)
    assert torch.equal(y, ref.skinny_gemm(x, ref.dequantize_fp8(Wq, scale), 1, 0))
    # e4m3 per-row quantisation: a few percent of the bf16 result, not garbage
    exact = ref.skinny_gemm(x, W, 1, 0).float()
    assert ((y.float() - exact).norm() / exact.norm()).item() < 0.1


def test_unsupported_forms_raise():
    W = (torch.randn(32, 128) * 0.05).to(torch.bfloat16)
    x = torch.randn(2, 128).to(torch.bfloat16)
    Wq, scale = ops.shuffle_weight_fp8(W)
    with pytest.raises(ValueError, match="x2"):
        ops.skinny_gemm(x, Wq, ops.PRO_NORM_ADD, ops.EPI_STORE, x2=x, wscale=scale)
    with pytest.raises(ValueError, match="split"):
        ops.skinny_gemm(x, Wq, wscale=scale, split_ws=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="rows"):
        ops.skinny_gemm(torch.zeros(33, 128, dtype=torch.bfloat16), Wq, wscale=scale)
    with pytest.raises(ValueError, match="wscale"):
        ops.skinny_gemm(x, Wq)                       # codes without scales: never a silent bf16 read
    with pytest.raises(ValueError, match="uint8"):
        ops.skinny_gemm(x, W, wscale=scale)
    with pytest.raises(ValueError, match="K %"):
        ops.shuffle_weight_fp8(torch.zeros(16, 96, dtype=torch.bfloat16))


def fp8_engine(model, **kw):
    cfg = dict(model=model, device="cpu", dtype="fp32", num_blocks=64, weights="random-full:5", weight_quant="fp8")
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


@pytest.mark.parametrize("model", ["tiny-llama-128", "tiny-qwen-128"])
def test_engine_fp8_cpu_greedy_turn(model):
    a, b = fp8_engine(model), fp8_engine(model)
    assert a.weight_residency == "fp8" and a.weight_quant == "fp8" and a.model.quant == "fp8"
    # single copy: the row-major linears are gone, the codes are uint8, the embedding is not quantised
    assert a.model.layers[0]["wqkv"] is None and a.model.w["lm_head"] is None
    d = a.model.decode_weights()
    assert d["layers"][0]["wqkv"].dtype == torch.uint8 and d["lm_head"].dtype == torch.uint8
    assert d["layers"][0]["wqkv_scale"].dtype == torch.float32
    assert a.model.w["embed"].dtype == a.dtype
    ta = a.run_turns([Turn("K", "Een ronde tafel met acht-bits gewichten.", GREEDY)])[0]
    tb = b.run_turns([Turn("K", "Een ronde tafel met acht-bits gewichten.", GREEDY)])[0]
    assert ta.error is None and len(ta.ids) == GREEDY.max_new_tokens
    assert ta.ids == tb.ids
    # the engine computes with bf16(code * scale): logits close to the bf16-weight engine's, not equal
    ref_e = Engine(EngineConfig(model=model, device="cpu", dtype="fp32", num_blocks=64, weights="random-full:5"))
    assert ref_e.weight_quant == "none"
    ids = a.encode_prompt("Een gedeelde sleutel voor de ronde tafel, graag. " * 2)
    la = a.prefill([(a.kv.seq("p"), ids)]).float()
    lr = ref_e.prefill([(ref_e.kv.seq("p"), ids)]).float()
    cos = torch.nn.functional.cosine_similarity(la.flatten(), lr.flatten(), dim=0).item()
    assert 0.9 < cos < 1.0 and not torch.equal(la, lr)


def test_env_default_and_explicit_none(monkeypatch):
    monkeypatch.setenv("ROUNDTABLE_WEIGHT_QUANT", "fp8")
    assert EngineConfig(model="tiny-llama-128").weight_quant == "fp8"
    assert EngineConfig(model="tiny-llama-128", weight_quant="none").weight_quant == "none"
    monkeypatch.delenv("ROUNDTABLE_WEIGHT_QUANT")
    assert EngineConfig(model="tiny-llama-128").weight_quant == "none"
    with pytest.raises(ConfigError):
        Engine(EngineConfig(model="tiny-llama-128", device="cpu", weight_quant="int4"))


def _config(quants):
    from theroundtaible_amd.types import RoundtableConfig
    knights = [{"name": f"Ridder{i}", "adapter": f"local-llm-r{i}", "capabilities": ["x"], "priority": i + 1}
               for i in range(len(quants))]
    return RoundtableConfig.from_dict({
        "version": "1.0", "project": "fp8", "language": "nl", "knights": knights,
        "rules": {"max_rounds": 1, "consensus_threshold": 9, "timeout_per_turn_seconds": 300,
                  "escalate_to_user_after": 5, "auto_execute": False, "ignore": [".git"], "round_mode": "parallel"},
        "chronicle": ".roundtable/chronicle.md",
        "engine": {"default_model": "tiny-llama-128", "max_new_tokens": 4, "ignore_eos": True, "temperature": 0.0,
                   "device": "cpu", "weights": "random-full:3"},
        "adapter_config": {f"local-llm-r{i}": {"engine": ({"weight_quant": q} if q else {})}
                           for i, q in enumerate(quants)}})


def test_config_plumbing_and_pool_keys(monkeypatch):
    from theroundtaible_amd.config import engine_settings
    from theroundtaible_amd.knights.registry import BackendFactory
    monkeypatch.delenv("ROUNDTABLE_WEIGHT_QUANT", raising=False)
    cfg = _config(["fp8", None, "fp8"])
    assert [engine_settings(cfg, f"local-llm-r{i}")["weight_quant"] for i in range(3)] == ["fp8", "none", "fp8"]
    factory = BackendFactory(cfg)
    b = [factory.create(f"local-llm-r{i}") for i in range(3)]
    # the knight's weight_quant reaches its EngineConfig; fp8 and bf16 knights of one model never share
    assert [x.engine.ecfg.weight_quant for x in b] == ["fp8", "none", "fp8"]
    assert b[0].engine is b[2].engine and b[0].engine is not b[1].engine
    assert len(factory.pool.engines) == 2
    assert b[0].engine.weight_residency == "fp8" and b[1].engine.weight_residency != "fp8"
    # an engine-wide setting applies to every knight; the environment only fills what is unstated
    cfg2 = _config([None, "none"])
    cfg2.raw["engine"]["weight_quant"] = "fp8"
    assert [engine_settings(cfg2, f"local-llm-r{i}")["weight_quant"] for i in range(2)] == ["fp8", "none"]
    monkeypatch.setenv("ROUNDTABLE_WEIGHT_QUANT", "fp8")
    cfg3 = _config([None, "none"])
    assert [engine_settings(cfg3, f"local-llm-r{i}")["weight_quant"] for i in range(2)] == ["fp8", "none"]
    cfg4 = _config(["int3"])
    with pytest.raises(ConfigError):
        engine_settings(cfg4, "local-llm-r0")


def test_refusals():
    from theroundtaible_amd.parallel.tp import TPInfo
    with pytest.raises(ConfigError, match="tensor parallel"):
        Engine(EngineConfig(model="tiny-llama-128", device="cpu", weight_quant="fp8"), TPInfo(size=2, rank=0))
    with pytest.raises(ConfigError, match="family"):
        Engine(EngineConfig(model="tiny-gpt2", device="cpu", weight_quant="fp8"))
    # a GEMM depth the 64-deep fp8 k-record does not divide: ffn 96
    with pytest.raises(ConfigError, match="k-record"):
        Engine(EngineConfig(model="tiny-llama-128", device="cpu", weight_quant="fp8", model_overrides={"ffn": 96}))
    assert math.gcd(96, ops.FP8_K_RECORD) != ops.FP8_K_RECORD
