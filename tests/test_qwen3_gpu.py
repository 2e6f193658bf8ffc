"""The Qwen3 family (``cfg.qk_norm``) on the GPU at the model level, on ``tiny-qwen3-128`` (4 heads x head_dim 128
over hidden 256, 1 KV head) with random weights and q_norm / k_norm gammas drawn away from ones: the fused decode
layer (qkv GEMM storing plain columns, then csrc/qk_norm_rope.hip: seven launches) against the unfused path for
every weight type and K/V page type, a 3-knight table that shares a prefix through a group, the captured step twice,
and the tensor-parallel fused path at tp 1."""
import pytest
import torch

from test_engine_gpu import _shared_turns
from theroundtaible_amd.engine import Engine, EngineConfig

pytestmark = pytest.mark.gpu
DEV = "cuda"


def qwen3_engine(**kw):
    cfg = dict(model="tiny-qwen3-128", weights="random-dev:5", device=DEV, num_blocks=64)
    cfg.update(kw)
    if cfg.get("kv_dtype") == "fp8":
        cfg.setdefault("kv_scale", {"k": 0.5, "v": [2.0, 0.25]})
    e = Engine(EngineConfig(**cfg))
    assert e.cfg.qk_norm and e.cfg.n_heads * e.cfg.head_dim == 2 * e.cfg.hidden
    g = torch.Generator(device=DEV).manual_seed(7)       # random init leaves the gammas at one: make them matter
    for lw in e.model.layers:
        for name in ("q_norm", "k_norm"):
            assert lw[name].shape == (128,)
            lw[name].copy_((1.0 + 0.3 * torch.randn(128, device=DEV, generator=g)).to(lw[name].dtype))
    return e


def decode_step(e, prompts):
    """-> (tokens, positions, meta) of one decode step over freshly prefilled sequences."""
    from theroundtaible_amd.models.llama import AttnMeta
    seqs = [e.kv.seq(f"s{i}") for i in range(len(prompts))]
    e.prefill([(s, e.encode_prompt(p)) for s, p in zip(seqs, prompts)])
    for s in seqs:
        e.kv.ensure_capacity(s, s.length + 1)
    pos = torch.tensor([s.length for s in seqs], device=DEV)
    slots = torch.tensor([s.blocks[p // 32] * 32 + p % 32 for s, p in zip(seqs, pos.tolist())], device=DEV)
    bt = torch.zeros(len(seqs), 8, dtype=torch.int32)
    for j, s in enumerate(seqs):
        bt[j, :len(s.blocks)] = torch.tensor(s.blocks)
    meta = AttnMeta("decode", slots, bt.to(DEV), (pos + 1).to(torch.int32), num_splits=4)
    return torch.tensor([5, 7, 11][:len(seqs)], device=DEV), pos, meta


@pytest.mark.parametrize("wq", ["none", "fp8", "mxfp4"])
@pytest.mark.parametrize("kvd", ["bf16", "fp8"])
def test_fused_decode_matches_unfused(wq, kvd):
    """The criterion of test_kv_fp8_gpu.py::test_fused_decode_matches_unfused: cosine > 0.999 per row."""
    e = qwen3_engine(weight_quant=wq, kv_dtype=kvd, use_graphs=False)
    assert (e.kv.k.dtype == torch.uint8) == (kvd == "fp8")
    tok, pos, meta = decode_step(e, ["fused versus unfused decode " * 4, "fused versus unfused decode " * 3])
    assert e.model.fused_decode_ok(tok)
    dec = e.model.decode_weights()["layers"][0]
    assert "q_norm" in dec and "bqkv" not in dec
    fused = e.model.forward(tok, pos, e.kv, meta).float()
    e.model.use_fused = False
    plain = e.model.forward(tok, pos, e.kv, meta).float()
    cos = torch.nn.functional.cosine_similarity(fused, plain, dim=-1)
    print(f"qwen3 weights {wq} kv {kvd}: fused vs unfused cosine min = {float(cos.min())}")
    assert float(cos.min()) > 0.999


def test_three_knights_share_a_prefix_and_the_captured_step_is_deterministic():
    outs = []
    for _ in range(2):
        e = qwen3_engine(num_blocks=512, use_graphs=True)
        assert e.ecfg.use_graphs
        _, turns = _shared_turns([], 1)
        r = e.run_turns(turns)
        assert all(o.error is None and o.metrics["shared_tokens"] > 0 and len(o.ids) == 16 for o in r)
        outs.append([o.ids for o in r])
    assert outs[0] == outs[1]


def test_tp_fused_path_at_tp1_gives_the_same_greedy_tokens():
    e = qwen3_engine(use_graphs=False)
    tok, pos, meta = decode_step(e, ["tensor parallel fused decode " * 4, "een tweede rij " * 5, "en een derde"])
    a = e.model.forward(tok, pos, e.kv, meta).float()
    e.model.force_tp_path = True
    b = e.model.forward(tok, pos, e.kv, meta).float()
    top2 = a.topk(2, dim=-1).values
    print(f"qwen3 tp path: cosine min {float(torch.nn.functional.cosine_similarity(a, b, dim=-1).min())}, "
          f"top-2 gaps {[round(float(x), 4) for x in top2[:, 0] - top2[:, 1]]}")
    assert a.argmax(-1).tolist() == b.argmax(-1).tolist()
    assert float(torch.nn.functional.cosine_similarity(a, b, dim=-1).min()) > 0.999
