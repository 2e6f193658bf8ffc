"""Per-head QK-norm + RoPE + K/V cache write (Qwen3) on the CPU: the fp32 reference (ops/reference.py
qk_norm_rope_and_cache) against the fp64 oracle (ops/oracle64.py qk_norm_rope) on every input of the GPU
kernel test, the measurement QKNORM_SLACK is built from, wrong variants that must land outside the
tolerance, and the detection / configuration of the Qwen3 family."""
import json
import math
import os

import pytest
import torch

from theroundtaible_amd.models.config import PRESETS, get_config
from theroundtaible_amd.ops import oracle64 as o64
from theroundtaible_amd.ops import reference as ref

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_COS_SIN = {}


def cos_sin_table(D):
    if D not in _COS_SIN:
        _COS_SIN[D] = ref.rope_cos_sin(o64.ROPE_MAX_POS, D, o64.ROPE_THETA)
    return _COS_SIN[D]


def cases():
    for hq, hkv, D in o64.QKNORM_SHAPES:
        for T in o64.QKNORM_T:
            for eps in o64.QKNORM_EPS:
                for rope in (True, False):
                    yield hq, hkv, D, T, eps, rope


def run_reference(qkv, gq, gk, eps, pos, table, slots, kc, vc, hq, hkv, D, dtype):
    """-> (q, written k) [T, heads, D] of ``dtype``: bf16 as the engine runs it, or fp32 copies of the same
    bf16 values (no bf16 rounding of the result: the reference's own arithmetic error)."""
    kc, vc = kc.to(dtype), vc.to(dtype)
    q = ref.qk_norm_rope_and_cache(qkv.to(dtype), gq.to(dtype), gk.to(dtype), eps, pos, table, kc, vc, slots, hq, hkv, D)
    return q, ref.k_rows(kc, torch.arange(o64.ROPE_BLOCKS))[slots], vc


def test_reference_vs_oracle_and_worst_is_recorded():
    worst, where = 0.0, None
    for hq, hkv, D, T, eps, rope in cases():
        qkv, pos, slots, kc0, vc0 = o64.qk_norm_case(hq, hkv, D, T)
        gq, gk = o64.qk_norm_gammas(D)
        table = cos_sin_table(D) if rope else None
        x = qkv[:, :(hq + hkv) * D].reshape(T, hq + hkv, D)
        e, mag = o64.qk_norm_rope(x, gq, gk, eps, table[pos] if rope else None, n_q=hq)
        tol = o64.qk_norm_tol(e, mag)
        what = f"qk_norm reference {(hq, hkv, D)} T={T} eps={eps} rope={rope}"
        q, k, vc = run_reference(qkv, gq, gk, eps, pos, table, slots, kc0, vc0, hq, hkv, D, BF)
        o64.assert_within(q, e[:, :hq], tol[:, :hq], what + " q")
        o64.assert_within(k, e[:, hq:], tol[:, hq:], what + " k")
        blk, off = slots // o64.ROPE_BS, slots % o64.ROPE_BS
        assert torch.equal(vc[blk, :, :, off], qkv[:, (hq + hkv) * D:].reshape(T, hkv, D)), what + " v"
        assert not bool(k[0, hkv - 1].any()) and bool(torch.isfinite(q.float()).all()), what + ": zero head / 2^60 head"
        q32, k32, _ = run_reference(qkv, gq, gk, eps, pos, table, slots, kc0, vc0, hq, hkv, D, torch.float32)
        d = (torch.cat([q32, k32], dim=1).double() - e).abs()
        ratio = torch.where(d > 0, d / mag, torch.zeros_like(d))
        if float(ratio.max()) > worst:
            worst, where = float(ratio.max()), what
    print(f"QKNORM_REF_WORST measured {worst:.3e} at {where}")
    assert worst <= o64.QKNORM_REF_WORST * 1.01, (worst, where)
    assert worst >= o64.QKNORM_REF_WORST * 0.5, "QKNORM_REF_WORST is not the measured value any more"
    assert o64.QKNORM_SLACK == 2.0 ** math.ceil(math.log2(4 * o64.QKNORM_REF_WORST))


# ---- teeth ----------------------------------------------------------------------------------------------

def wrong(kind, x, n_q, gq, gk, eps, cs):
    """fp32 q | k [T, heads, D] (bf16) of a deliberately wrong kernel."""
    xf = x.float()
    D = x.shape[-1]
    g = torch.cat([gq.float().expand(n_q, D), (gq if kind == "q_gamma_for_k" else gk).float().expand(x.shape[1] - n_q, D)])
    rot = (lambda t: ref._rotate(t, cs)) if cs is not None else (lambda t: t)
    if kind == "norm_after_rope":
        xr = rot(xf)
        return (xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + eps) * g).to(BF)
    ms = xf.pow(2).mean((-2, -1), keepdim=True) if kind == "row_mean" else xf.pow(2).mean(-1, keepdim=True)
    y = xf * torch.rsqrt(ms + (0.0 if kind == "no_eps" else eps)) * g
    if kind == "bf16_between":
        y = y.to(BF).float()
    return rot(y).to(BF)


@pytest.mark.parametrize("kind", ["norm_after_rope", "row_mean", "q_gamma_for_k", "no_eps", "bf16_between"])
def test_wrong_variants_land_outside_the_tolerance(kind):
    """Each wrong variant is more than 4 tolerances off on at least one element of the (32, 8, 128), T = 37
    input; the right fp32 computation (kind None) is inside."""
    hq, hkv, D, T, eps = 32, 8, 128, 37, 1e-6
    qkv, pos, _, _, _ = o64.qk_norm_case(hq, hkv, D, T)
    gq, gk = o64.qk_norm_gammas(D)
    cs = cos_sin_table(D)[pos]
    x = qkv[:, :(hq + hkv) * D].reshape(T, hq + hkv, D)
    e, mag = o64.qk_norm_rope(x, gq, gk, eps, cs, n_q=hq)
    tol = o64.qk_norm_tol(e, mag)
    assert o64.error_ratio(wrong(None, x, hq, gq, gk, eps, cs), e, tol) <= 1.0
    r = o64.error_ratio(wrong(kind, x, hq, gq, gk, eps, cs), e, tol)
    print(f"wrong variant {kind}: error / tolerance {r:.1f}")
    assert r > 4.0, (kind, r)


# ---- detection and configuration ------------------------------------------------------------------------

QWEN3_8B = {"model_type": "qwen3", "hidden_size": 4096, "num_hidden_layers": 36, "num_attention_heads": 32,
            "num_key_value_heads": 8, "head_dim": 128, "intermediate_size": 12288, "vocab_size": 151936,
            "max_position_embeddings": 40960, "rope_theta": 1000000.0, "rms_norm_eps": 1e-6,
            "tie_word_embeddings": False, "attention_bias": False, "use_sliding_window": False,
            "layer_types": ["full_attention"] * 36}


def detect(tmp_path, hf):
    from theroundtaible_amd.utils.local_detect import checkpoint_model
    (tmp_path / "config.json").write_text(json.dumps(hf))
    return checkpoint_model(str(tmp_path))


def test_qwen3_config_maps_to_a_qwen3_preset(tmp_path):
    preset, ov = detect(tmp_path, QWEN3_8B)
    assert preset == "qwen3-8b" and ov == {}
    assert get_config(preset, **ov).qk_norm and not get_config(preset, **ov).qkv_bias
    # head_dim comes from the file, not from hidden / heads (0.6B: 1024 / 16 = 64, head_dim 128)
    small = dict(QWEN3_8B, hidden_size=1024, num_hidden_layers=28, num_attention_heads=16, intermediate_size=3072,
                 tie_word_embeddings=True, layer_types=["full_attention"] * 28)
    preset, ov = detect(tmp_path, small)
    cfg = get_config(preset, **ov)
    assert preset == "qwen3-0.6b" and cfg.head_dim == 128 and cfg.qk_norm
    # any shape lands in the family
    odd = dict(QWEN3_8B, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
               head_dim=64, intermediate_size=512, vocab_size=32000, layer_types=None)
    preset, ov = detect(tmp_path, odd)
    assert preset.startswith("qwen3-") and get_config(preset, **ov).qk_norm and get_config(preset, **ov).head_dim == 64


@pytest.mark.parametrize("change", [{"attention_bias": True}, {"use_sliding_window": True},
                                    {"layer_types": ["full_attention"] * 35 + ["sliding_attention"]},
                                    {"model_type": "qwen3_moe"}],
                         ids=["attention_bias", "sliding_window", "layer_types", "qwen3_moe"])
def test_qwen3_refusals(tmp_path, change):
    assert detect(tmp_path, dict(QWEN3_8B, **change)) is None


def test_qwen2_config_is_unaffected(tmp_path):
    hf = {"model_type": "qwen2", "hidden_size": 3584, "num_hidden_layers": 28, "num_attention_heads": 28,
          "num_key_value_heads": 4, "intermediate_size": 18944, "vocab_size": 152064, "max_position_embeddings": 32768,
          "rope_theta": 1000000.0, "rms_norm_eps": 1e-6, "tie_word_embeddings": False}
    preset, ov = detect(tmp_path, hf)
    assert preset == "qwen2.5-7b" and ov == {}
    cfg = get_config(preset, **ov)
    assert cfg.qkv_bias and not cfg.qk_norm


def test_presets_and_param_count():
    for name in ("qwen3-0.6b", "qwen3-1.7b", "qwen3-4b", "qwen3-8b", "qwen3-14b", "qwen3-32b", "tiny-qwen3",
                 "tiny-qwen3-128"):
        cfg = PRESETS[name]
        assert cfg.qk_norm and not cfg.qkv_bias and cfg.arch == "llama" and cfg.head_dim in (64, 128)
        assert cfg.rope_theta == 1e6 and cfg.norm_eps == 1e-6
        assert cfg.n_params() - get_config(name, qk_norm=False).n_params() == cfg.n_layers * 2 * cfg.head_dim
    assert [PRESETS[n].tie_embeddings for n in ("qwen3-0.6b", "qwen3-1.7b", "qwen3-4b", "qwen3-8b")] == [True, True,
                                                                                                         True, False]
    t = PRESETS["tiny-qwen3-128"]
    assert t.n_heads * t.head_dim == 512 and t.hidden == 256
    assert not any(c.qk_norm for n, c in PRESETS.items() if "qwen3" not in n)


def test_layout_and_hf_names():
    from theroundtaible_amd.models.weights import _hf_llama_name_map, llama_layout
    cfg = PRESETS["tiny-qwen3-128"]
    lay = llama_layout(cfg)
    assert lay["layers.1.q_norm"] == ((128,), "ones", None) and lay["layers.0.k_norm"] == ((128,), "ones", None)
    assert lay["layers.0.wo"][0] == (256, 512) and "layers.0.bqkv" not in lay
    names = _hf_llama_name_map(cfg)
    t = {"model.layers.1.self_attn.q_norm.weight": 1, "model.layers.1.self_attn.k_norm.weight": 2}
    assert names["layers.1.q_norm"](t) == 1 and names["layers.1.k_norm"](t) == 2
    assert "layers.0.q_norm" not in llama_layout(PRESETS["tiny-qwen"])


def test_aliases_resolve():
    from theroundtaible_amd.config import resolve_model_name
    for size in ("0.6b", "1.7b", "4b", "8b", "14b", "32b"):
        for name in (f"qwen3-{size}", f"Qwen/Qwen3-{size.upper()}", f"qwen-3-{size}-instruct"):
            assert resolve_model_name(name, "tiny-llama") == f"qwen3-{size}", name
    assert resolve_model_name("qwen3-30b-a3b", "tiny-llama") == "tiny-llama"
    assert resolve_model_name("meta-llama-3-8b", "tiny-llama") == "llama3-8b"


def test_example_config_loads():
    from theroundtaible_amd.config import engine_settings, validate_config
    from theroundtaible_amd.types import RoundtableConfig
    raw = json.load(open(os.path.join(ROOT, "examples", "config.qwen3.json")))
    validate_config(raw)
    rc = RoundtableConfig.from_dict(raw)
    models = {k.name: engine_settings(rc, k.adapter)["model"] for k in rc.knights}
    assert models == {"Claude": "llama3-8b", "Gemini": "qwen3-8b", "GPT": "llama3-8b"}
    assert get_config(models["Gemini"]).qk_norm
