"""Numerical parity with Hugging Face ``transformers`` for the Qwen3 family (tests/test_hf_parity.py's checks on a
tiny ``Qwen3ForCausalLM`` written with ``save_pretrained``): the Llama block without q/k/v biases plus an RMSNorm
over head_dim on every q and k head before RoPE (``self_attn.q_norm`` / ``k_norm``, one ``[head_dim]`` weight each
per layer). The norm weights are drawn away from HF's initial ones, which would hide a swapped or missing gamma.
Without the family in utils/local_detect.py these tests fail at ``resolve_model``."""
import pytest
import torch

transformers = pytest.importorskip("transformers")

from test_hf_parity import _check_cpu, _check_gpu, _sharpen  # noqa: E402

from theroundtaible_amd.models.config import get_config  # noqa: E402


def _save_qwen3(path, big=False, seed=0):
    """``big``: head_dim 128 with 4 heads over hidden 256 (heads x head_dim = 512 != hidden, as Qwen3-0.6B and
    Qwen3-4B have it) and 1 KV head; else head_dim 64, 2 KV heads, tied embeddings."""
    kw = dict(hidden_size=256, intermediate_size=1024 if big else 512, num_hidden_layers=2, num_attention_heads=4,
              num_key_value_heads=1 if big else 2, head_dim=128 if big else 64, vocab_size=32000,
              max_position_embeddings=8192 if big else 4096, rms_norm_eps=1e-6, rope_theta=1e6,
              tie_word_embeddings=not big, initializer_range=0.08, use_sliding_window=False, attention_bias=False)
    torch.manual_seed(seed)
    m = transformers.Qwen3ForCausalLM(transformers.Qwen3Config(**kw))
    _sharpen(m)
    with torch.no_grad():
        for layer in m.model.layers:
            layer.self_attn.q_norm.weight.normal_(1.0, 0.3)
            layer.self_attn.k_norm.weight.normal_(1.0, 0.3)
    m.eval().save_pretrained(str(path), safe_serialization=True)
    return m


def test_qwen3_matches_transformers(tmp_path):
    """head_dim 64, tied embeddings; config.json alone maps it to the Qwen3 family."""
    from theroundtaible_amd.utils.local_detect import checkpoint_model
    hf = _save_qwen3(tmp_path)
    preset, ov = checkpoint_model(str(tmp_path))
    cfg = get_config(preset, **ov)
    assert preset.startswith("qwen3-") and cfg.qk_norm and not cfg.qkv_bias and cfg.head_dim == 64
    _check_cpu("tiny-qwen3", hf, tmp_path)


def test_qwen3_head_dim_128_over_hidden_256_matches_transformers(tmp_path):
    """heads x head_dim = 512 over hidden 256: the o projection is [256, 512]."""
    from theroundtaible_amd.utils.local_detect import checkpoint_model
    hf = _save_qwen3(tmp_path, big=True)
    preset, ov = checkpoint_model(str(tmp_path))
    cfg = get_config(preset, **ov)
    assert cfg.head_dim == 128 and cfg.hidden == 256 and cfg.n_heads == 4 and cfg.qk_norm
    _check_cpu("tiny-qwen3-128", hf, tmp_path)


def test_missing_qk_norm_is_detected(tmp_path):
    """The parity check is sensitive to the QK-norm: the same checkpoint run as a plain Llama block fails."""
    hf = _save_qwen3(tmp_path)
    with pytest.raises(AssertionError):
        _check_cpu("tiny-qwen3", hf, tmp_path, {"qk_norm": False})


@pytest.mark.gpu
def test_qwen3_gpu_kernels_match_transformers(tmp_path):
    """Qwen3 on the HIP path: prefill through K2n, fused decode (qkv GEMM storing plain columns, then K2n) in
    the captured graphs."""
    _check_gpu("tiny-qwen3-128", _save_qwen3(tmp_path, big=True), tmp_path)
