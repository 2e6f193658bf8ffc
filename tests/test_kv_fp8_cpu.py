"""The FP8 K/V cache (kv_dtype "fp8") without a GPU: the scalar rule of ops/reference.py (kv_fp8_code /
kv_fp8_value), the attention bound on fp8 twins of the oracle cases (sound for an fp32 emulation of the fp8
decode path, sharp against four wrong variants), configuration and refusals, and the CPU engine on an fp8 pool.

The emulation pieces (tile loop, state merge, split ranges) are the ones of tests/test_attention_oracle_cpu.py."""
import math

import pytest
import torch

from test_attention_oracle_cpu import (LOG2E, emu_tiles, empty_state, merge_state, split_ranges)
from theroundtaible_amd import ops
from theroundtaible_amd.config import engine_settings, resolve_kv_dtype, resolve_kv_scale
from theroundtaible_amd.engine import Engine, EngineConfig, SamplingParams, Turn
from theroundtaible_amd.engine.kv_cache import PagedKVCache
from theroundtaible_amd.errors import ConfigError
from theroundtaible_amd.ops import oracle64 as o64
from theroundtaible_amd.ops import reference as ref
from theroundtaible_amd.prompt import Prompt

BF = torch.bfloat16
SCALES = ((1.0, 1.0), (0.5, 4.0), (0.37, 2.9))
GREEDY = SamplingParams(temperature=0.0, max_new_tokens=10, ignore_eos=True, stop_on_consensus=False)


# ---- the rule -----------------------------------------------------------------------------------

def finite_bf16() -> torch.Tensor:
    y = o64.finite_bf16_table().float()
    assert y.numel() == 65280
    return y


def e4m3_step(x: torch.Tensor) -> torch.Tensor:
    """The e4m3 step at magnitude |x|: 2^(max(floor(log2 |x|), -6) - 3)."""
    ex = torch.floor(torch.log2(x.abs().double().clamp_min(2.0 ** -60))).clamp_min(-6.0)
    return torch.exp2(ex - 3.0)


@pytest.mark.parametrize("scale", [1.0, 4.0, 0.37])      # inverse scales 1, 0.25, 1 / 0.37
def test_code_rule_over_every_finite_bf16(scale):
    y = finite_bf16()
    inv = ref.kv_fp8_inv(scale)
    codes = ref.kv_fp8_code(y, inv)
    val = ref.kv_fp8_value(codes).double()
    x = (y * inv).double()                                # the ONE fp32 multiply, exactly as rounded
    assert bool(torch.isfinite(val).all())                # no finite input reaches the NaN code
    # monotone: sorted inputs give sorted values
    order = torch.argsort(x, stable=True)
    assert bool((val[order][1:] >= val[order][:-1]).all())
    # within half a step below saturation, exactly +-448 from 448 upward
    sat = x.abs() >= 448.0
    assert bool(sat.any()) and bool((val[sat] == 448.0 * torch.sign(x[sat])).all())
    err = (val - x).abs()[~sat]
    assert bool((err <= 0.5 * e4m3_step(x[~sat])).all())
    # ties go to even: where the error is exactly half a step, the kept mantissa bit 0 is clear
    tie = torch.zeros_like(sat)
    tie[~sat] = err == 0.5 * e4m3_step(x[~sat])
    if scale != 0.37:
        assert bool(tie.any())                            # bf16 has 7 mantissa bits: exact ties exist
    assert bool((codes[tie] & 1 == 0).all())
    # the sign bit is the input's, zero included
    assert bool(((codes >> 7).bool() == torch.signbit(y)).all())


def test_code_rule_specials():
    inf, nan = float("inf"), float("nan")
    t = torch.tensor([inf, -inf, nan, 448.0, 464.0, 1e30, -1e30, 0.0, -0.0, 17.0, 19.0])
    c = ref.kv_fp8_code(t, 1.0).tolist()
    assert c == [0x7E, 0xFE, 0x7F, 0x7E, 0x7E, 0x7E, 0xFE, 0x00, 0x80, 0x58, 0x5A]   # 17 -> 16, 19 -> 20
    assert ref.kv_fp8_code(torch.tensor([inf, nan]), 0.25).tolist() == [0x7E, 0x7F]
    v = ref.kv_fp8_value(torch.tensor([0, 0x7E, 0xFE, 0x58, 0x5A], dtype=torch.uint8), 2.0)
    assert v.tolist() == [0.0, 896.0, -896.0, 32.0, 40.0]
    assert math.isnan(float(ref.kv_fp8_value(torch.tensor([0x7F], dtype=torch.uint8))))
    # zero bytes are a finite +0: the zero-initialised pool's masked tail keys stay finite
    z = ref.kv_fp8_value(torch.zeros(4, dtype=torch.uint8), 3.0)
    assert bool((z == 0).all()) and not bool(torch.signbit(z).any())
    # e4m3 is a subset of bf16: the convert to bf16 is exact for every code
    allc = torch.arange(256, dtype=torch.int64).to(torch.uint8)
    v = ref.kv_fp8_value(allc)
    ok = ~torch.isnan(v)
    assert bool((v[ok].to(BF).float() == v[ok]).all())


def test_fp8_block_layout_roundtrip_and_mixed_dtypes():
    nb, hkv, bs, d = 3, 2, 32, 128
    k8 = torch.zeros(nb, hkv, bs, d, dtype=torch.uint8)
    v8 = torch.zeros(nb, hkv, d, bs, dtype=torch.uint8)
    g = torch.Generator().manual_seed(3)
    codes = torch.randint(0, 256, (nb * bs, hkv, d), dtype=torch.uint8, generator=g)
    blk, off = torch.arange(nb).repeat_interleave(bs), torch.arange(bs).repeat(nb)
    ref.write_k_fp8(k8, blk, off, codes)
    ref.write_v_fp8(v8, blk, off, codes)
    assert torch.equal(ref.k_rows_fp8(k8, torch.arange(nb)), codes)
    assert torch.equal(ref.v_rows_fp8(v8, torch.arange(nb)), codes)
    # the byte addresses are csrc/common.h kc8_elem / vc8_elem
    kb, vb = k8[1, 1].reshape(-1), v8[1, 1].reshape(-1)
    for key in (0, 5, 8, 31):
        for dd in (0, 15, 16, 17, 63, 64, 100, 127):
            ka = (dd >> 6) * (bs * 64) + key * 64 + (dd & 63)
            va = (dd >> 5) * (32 * bs) + (dd & 15) * (2 * bs) + (key >> 3) * 16 + ((dd >> 4) & 1) * 8 + (key & 7)
            assert kb[ka] == codes[bs + key, 1, dd] and vb[va] == codes[bs + key, 1, dd]
    with pytest.raises(ValueError, match="mixed"):
        ref.is_fp8_cache(k8, torch.zeros(nb, hkv, d, bs, dtype=BF))


# ---- the attention bound on fp8 twins -----------------------------------------------------------------

def twin_rows(tw, s, variant=None):
    """K, V of every entry of block-table row ``s`` as the fp8 decode kernel's MFMAs see them: the
    UNSCALED e4m3 values (exact in bf16), fp32. ``variant``: a wrong reading of the bytes."""
    n = tw.block_tables.shape[1] * o64.ATTN_BS
    blocks = tw.block_tables[s][:n // o64.ATTN_BS].long()
    if variant == "bf16_order":          # the bf16 chunk-major map (kc_elem) applied to the fp8 K block
        kc = ref.k_rows(tw.k_cache, blocks)
    else:
        kc = ref.k_rows_fp8(tw.k_cache, blocks)
    vc = ref.v_rows_fp8(tw.v_cache, blocks)
    if variant == "e5m2":
        return kc.view(torch.float8_e5m2).float(), vc.view(torch.float8_e5m2).float()
    return ref.kv_fp8_value(kc), ref.kv_fp8_value(vc)


def emu_decode_fp8(tw, splits, variant=None):
    """fp32 emulation of the fp8 decode path: the convert (exact), k_scale folded into the softmax
    scale (scale * k_scale * log2 e in fp32), bf16 P, v_scale folded into the final 1/l."""
    bs, hq, hkv, d = o64.ATTN_BS, tw.hq, tw.hkv, tw.d
    G = hq // hkv
    ks, vs = tw.k_scale, tw.v_scale
    if variant == "swapped":
        ks, vs = vs, ks
    if variant == "no_v_scale":
        vs = 1.0
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)      # noqa: E731
    sl2 = f32(tw.scale) * f32(ks) * LOG2E
    groups, _ = ops.decode_groups(tw.group_of, tw.shared, G)
    out = torch.empty_like(tw.q)
    for b in range(tw.q.shape[0]):
        ctx = int(tw.ctx_lens[b])
        b0, n, sh = (int(x) for x in groups[b])
        k, v = twin_rows(tw, b, variant)
        if not bool(torch.isfinite(k).all() and torch.isfinite(v).all()):       # e5m2 has inf / NaN codes
            k, v = torch.nan_to_num(k, 0.0, 57344.0, -57344.0), torch.nan_to_num(v, 0.0, 57344.0, -57344.0)
        qf = tw.q[b].float().reshape(1, hkv, G, d)
        M, L, O = empty_state(1, hkv, G, d)
        for tiles in split_ranges(ctx, b, b0, n, sh, splits):
            tl = [(t * bs, t * bs + bs, t * bs) for t in tiles]
            M, L, O = merge_state(M, L, O, *emu_tiles(qf, k, v, torch.tensor([ctx]), tl, sl2))
        inv = torch.where(L > 0, 1.0 / L, torch.zeros_like(L)) * f32(vs)
        out[b] = (O * inv[..., None]).to(BF).reshape(hq, d)
    return out


@pytest.mark.parametrize("scales", SCALES)
@pytest.mark.parametrize("kind", o64.ATTN_KINDS)
def test_fp8_decode_emulation_within_attn_tol(kind, scales):
    """Sound: no new tolerance. (8, 1, 128) is the copy-loop / GM 8 configuration, 3 splits."""
    tw = o64.attn_case_fp8(o64.attn_decode_case(kind, 8, 1, 128), *scales)
    assert tw.k_cache.dtype == torch.uint8 and tw.v_cache.dtype == torch.uint8
    e, A, tol = o64.attn_oracle(tw)
    o64.assert_within(emu_decode_fp8(tw, 3), e, tol, f"fp8 twin {kind} {scales}")
    # the torch reference reads the same bytes through the same layout and scales
    got = ref.paged_attention_decode(tw.q, tw.k_cache, tw.v_cache, tw.block_tables, tw.ctx_lens, tw.scale, *scales)
    o64.assert_within(got, e, tol, f"fp8 reference {kind} {scales}")


def test_fp8_grouped_and_wide_emulation_within_attn_tol():
    for cfg, case in (((32, 8, 128), o64.attn_group_case("random", 32, 8, 128)),
                      ((28, 4, 128), o64.attn_decode_case("peaky", 28, 4, 128))):
        tw = o64.attn_case_fp8(case, 0.37, 2.9)
        e, A, tol = o64.attn_oracle(tw)
        o64.assert_within(emu_decode_fp8(tw, 3), e, tol, f"fp8 twin {cfg}")


def test_fp8_twin_poison_is_finite_and_placed():
    case = o64.attn_decode_case("random", 8, 1, 128)
    tw = o64.attn_case_fp8(case, 0.37, 2.9)
    assert bool(torch.isfinite(tw.k_deq).all()) and bool(torch.isfinite(tw.v_deq).all())
    pb = torch.tensor([tw.poison_block])
    v = ref.kv_fp8_value(ref.v_rows_fp8(tw.v_cache, pb), 2.9)
    want = float(ref.kv_fp8_value(ref.kv_fp8_code(torch.tensor([o64.ATTN_POISON_V]), ref.kv_fp8_inv(2.9)), 2.9))
    assert bool((v == want).all()) and 80.0 < want < 112.0
    # the twin's codes are kv_fp8_code's own except the nonzero V values it would round to the zero code
    # (lifted to +-2^-9, see attn_case_fp8): |N(0,1)| / 2.9 < 2^-10 has probability 0.23 %, so well under
    # 1 % of the V bytes, every one of them the code 0x01 / 0x81, and none where V is exactly 0 (census)
    nb, hkv, bs, d = case.k_cache.shape
    V = case.v_cache.permute(0, 3, 1, 2).reshape(nb * bs, hkv, d).float()
    own = ref.kv_fp8_code(V, ref.kv_fp8_inv(2.9))
    got = ref.v_rows_fp8(tw.v_cache, torch.arange(nb))
    diff = own != got
    assert int(diff.sum()) == tw.v_lifted and 0 < tw.v_lifted < 0.01 * V.numel()
    assert bool(((got[diff] & 0x7F) == 1).all()) and bool(((own[diff] & 0x7F) == 0).all())
    Kc = ref.kv_fp8_code(ref.k_rows(case.k_cache, torch.arange(nb)).float(), ref.kv_fp8_inv(0.37))
    assert torch.equal(ref.k_rows_fp8(tw.k_cache, torch.arange(nb)), Kc)          # K: untouched
    assert o64.attn_case_fp8(o64.attn_decode_case("census", 8, 1, 128), 0.37, 2.9).v_lifted == 0
    # the oracle of the twin at scale 1 differs from the bf16 case's only by the quantisation of K / V
    t1 = o64.attn_case_fp8(case)
    e8, _, _ = o64.attn_oracle(t1)
    e16, _, _ = o64.attn_oracle(case)
    assert 0 < float((e8 - e16).abs().max()) < 0.25


# Wrong variants, each on the "random" rows of (8, 1, 128) — and "peaky" for the layout one — at scales
# (0.5, 4): scales of (1, 1) cannot separate an omitted or swapped scale, and "census" (K = 0) cannot
# separate a wrong K layout, so neither is used here.
VARIANTS = {"no_v_scale": "random", "swapped": "random", "e5m2": "random", "bf16_order": "peaky"}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_fp8_wrong_variant_is_caught(variant):
    tw = o64.attn_case_fp8(o64.attn_decode_case(VARIANTS[variant], 8, 1, 128), 0.5, 4.0)
    e, A, tol = o64.attn_oracle(tw)
    o64.assert_within(emu_decode_fp8(tw, 3), e, tol, "unmutated")
    r = o64.error_ratio(emu_decode_fp8(tw, 3, variant), e, tol)
    print(f"{variant} on fp8 decode (8, 1, 128) {VARIANTS[variant]} scales (0.5, 4): error / tolerance {r:.1f}")
    assert r > 4.0


# ---- configuration ------------------------------------------------------------------------------------

def _config(dtypes, engine=None):
    from theroundtaible_amd.types import RoundtableConfig
    knights = [{"name": f"Ridder{i}", "adapter": f"local-llm-r{i}", "capabilities": ["x"], "priority": i + 1}
               for i in range(len(dtypes))]
    eng = {"default_model": "tiny-llama-128", "max_new_tokens": 4, "ignore_eos": True, "temperature": 0.0,
           "device": "cpu", "weights": "random-full:3"}
    eng.update(engine or {})
    return RoundtableConfig.from_dict({
        "version": "1.0", "project": "kvfp8", "language": "nl", "knights": knights,
        "rules": {"max_rounds": 1, "consensus_threshold": 9, "timeout_per_turn_seconds": 300,
                  "escalate_to_user_after": 5, "auto_execute": False, "ignore": [".git"], "round_mode": "parallel"},
        "chronicle": ".roundtable/chronicle.md", "engine": eng,
        "adapter_config": {f"local-llm-r{i}": {"engine": ({"kv_dtype": q} if q else {})}
                           for i, q in enumerate(dtypes)}})


def test_kv_dtype_resolution_and_two_engines(monkeypatch):
    from theroundtaible_amd.knights.registry import BackendFactory
    monkeypatch.delenv("ROUNDTABLE_KV_DTYPE", raising=False)
    assert resolve_kv_dtype(None) == "bf16" and resolve_kv_dtype("FP8") == "fp8" and resolve_kv_dtype("bfloat16") == "bf16"
    assert EngineConfig(model="tiny-llama-128").kv_dtype == "bf16"
    cfg = _config(["fp8", None, "fp8"])
    assert [engine_settings(cfg, f"local-llm-r{i}")["kv_dtype"] for i in range(3)] == ["fp8", "bf16", "fp8"]
    factory = BackendFactory(cfg)
    b = [factory.create(f"local-llm-r{i}") for i in range(3)]
    assert [x.engine.kv_dtype for x in b] == ["fp8", "bf16", "fp8"]
    # a bf16-KV knight and an fp8-KV knight of one model get two engines; equal settings share one
    assert b[0].engine is b[2].engine and b[0].engine is not b[1].engine and len(factory.pool.engines) == 2
    assert b[0].engine.kv.k.dtype == torch.uint8 and b[1].engine.kv.k.dtype != torch.uint8
    # engine-wide applies to every knight that states nothing; a knight's own word wins
    cfg2 = _config([None, "bf16"], {"kv_dtype": "fp8", "kv_scale": {"k": 0.5, "v": [2.0, 4.0]}})
    st = [engine_settings(cfg2, f"local-llm-r{i}") for i in range(2)]
    assert [s["kv_dtype"] for s in st] == ["fp8", "bf16"] and st[0]["kv_scale"] == {"k": 0.5, "v": [2.0, 4.0]}
    e = BackendFactory(cfg2).create("local-llm-r0").engine
    assert e.kv.scales(0) == (0.5, 2.0) and e.kv.scales(1) == (0.5, 4.0)
    # the environment only fills what no config states
    monkeypatch.setenv("ROUNDTABLE_KV_DTYPE", "fp8")
    cfg3 = _config([None, "bf16"])
    assert [engine_settings(cfg3, f"local-llm-r{i}")["kv_dtype"] for i in range(2)] == ["fp8", "bf16"]
    assert EngineConfig(model="tiny-llama-128").kv_dtype == "fp8"
    assert EngineConfig(model="tiny-llama-128", kv_dtype="bf16").kv_dtype == "bf16"
    monkeypatch.delenv("ROUNDTABLE_KV_DTYPE")
    with pytest.raises(ConfigError, match="kv_dtype"):
        engine_settings(_config(["int8"]), "local-llm-r0")
    # kv_scale is read only with an fp8 cache: a stray (even bad) one beside bf16 pages raises nothing
    stray = _config([None, "fp8"], {"kv_scale": {"k": -1.0}})
    assert engine_settings(stray, "local-llm-r0")["kv_dtype"] == "bf16"
    assert BackendFactory(stray).create("local-llm-r0").engine.kv.scales(0) == (1.0, 1.0)
    with pytest.raises(ConfigError, match="kv_dtype"):
        engine_settings(stray, "local-llm-r1")


def test_serve_cli_takes_kv_dtype():
    from theroundtaible_amd.cli import build_parser
    args = build_parser().parse_args(["serve", "--kv-dtype", "fp8"])
    assert args.kv_dtype == "fp8"
    assert build_parser().parse_args(["serve"]).kv_dtype is None


def test_refusals_name_kv_dtype():
    from theroundtaible_amd.parallel.tp import TPInfo
    mk = lambda **kw: EngineConfig(**{**dict(model="tiny-llama-128", device="cpu", dtype="fp32", kv_dtype="fp8",   # noqa: E731
                                             num_blocks=64), **kw})
    with pytest.raises(ConfigError, match="kv_dtype.*tensor parallel"):
        Engine(mk(), TPInfo(size=2, rank=0))
    with pytest.raises(ConfigError, match="kv_dtype.*gpt2"):
        Engine(mk(model="tiny-gpt2"))
    with pytest.raises(ConfigError, match="kv_dtype.*head_dim"):
        Engine(mk(model="tiny-llama"))                                   # head_dim 64
    with pytest.raises(ConfigError, match="kv_dtype.*group"):
        Engine(mk(model_overrides={"n_heads": 16, "hidden": 2048}))      # 16 query heads on 1 kv head
    for bad in ({"k": 0.0}, {"v": -1.0}, {"k": float("inf")}, {"v": float("nan")}, {"k": [1.0]}, {"k": [1.0, 0.0]},
                {"q": 1.0}, {"k": "1"}, {"k": True}):
        with pytest.raises(ConfigError, match="kv_dtype"):
            Engine(mk(kv_scale=bad))
    with pytest.raises(ConfigError, match="kv_dtype"):
        resolve_kv_scale({"k": -2})
    with pytest.raises(ConfigError, match="kv_dtype"):
        Engine(mk(kv_dtype="fp4"))


def test_bytes_per_block_halves_and_pool_doubles():
    assert PagedKVCache.bytes_per_block(2, 1, 128, 32, 1) * 2 == PagedKVCache.bytes_per_block(2, 1, 128, 32, 2)
    mk = lambda kvd: Engine(EngineConfig(model="tiny-llama-128", device="cpu", dtype="bf16", kv_dtype=kvd,   # noqa: E731
                                         kv_budget_bytes=8 << 20, weights="random:1"))
    a, b = mk("bf16"), mk("fp8")
    assert b.kv_bytes_per_token() * 2 == a.kv_bytes_per_token()
    assert b.kv_capacity_tokens == 2 * a.kv_capacity_tokens
    assert b.kv.k.element_size() == 1 and b.kv.k.numel() == 2 * a.kv.k.numel()


# ---- the CPU engine on an fp8 pool --------------------------------------------------------------------

def fp8_engine(**kw):
    cfg = dict(model="tiny-llama-128", device="cpu", dtype="fp32", num_blocks=128, weights="random:2", kv_dtype="fp8",
               kv_scale={"k": 0.5, "v": [2.0, 0.25]})
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


def test_cpu_engine_greedy_is_deterministic_and_uses_the_codes():
    a, b = fp8_engine(), fp8_engine()
    ta = a.run_turns([Turn("K", "Een ronde tafel met acht-bits sleutels.", GREEDY)])[0]
    tb = b.run_turns([Turn("K", "Een ronde tafel met acht-bits sleutels.", GREEDY)])[0]
    assert ta.error is None and len(ta.ids) == GREEDY.max_new_tokens and ta.ids == tb.ids
    assert a.kv.k.dtype == torch.uint8 and int(a.kv.k.count_nonzero()) > 0 and int(a.kv.v.count_nonzero()) > 0
    # close to, and not equal to, the bf16-KV engine: the cache really is quantised
    r = Engine(EngineConfig(model="tiny-llama-128", device="cpu", dtype="fp32", num_blocks=128, weights="random:2"))
    ids = a.encode_prompt("Een gedeelde sleutel voor de ronde tafel, graag. " * 3)
    la = a.prefill([(a.kv.seq("p"), ids)]).float()
    lr = r.prefill([(r.kv.seq("p"), ids)]).float()
    # prefill attention reads the keys it has just written: quantised in one engine, not in the other
    cos = torch.nn.functional.cosine_similarity(la.flatten(), lr.flatten(), dim=0).item()
    assert 0.9 < cos < 1.0 and not torch.equal(la, lr)


def test_cpu_engine_fork_cow_truncate_keep_codes():
    e = fp8_engine()
    t1 = e.run_turns([Turn("A", "Onderwerp: caching in de tafel, met codes.", GREEDY)])[0]
    kv = e.kv
    s = kv.seqs["A"]
    before = [kv.k[:, b].clone() for b in s.blocks], [kv.v[:, b].clone() for b in s.blocks]
    f = kv.fork("A", "B")
    assert f.blocks == s.blocks
    assert f.length % kv.block_size                  # a shared partial tail block: the writer copies it
    kv.ensure_capacity(f, f.length + 1)
    if f.length % kv.block_size:
        assert f.blocks[-1] != s.blocks[-1]
        assert torch.equal(kv.k[:, f.blocks[-1]], kv.k[:, s.blocks[-1]]) and \
            torch.equal(kv.v[:, f.blocks[-1]], kv.v[:, s.blocks[-1]])
    d = kv.fork("A", "C", copy=True)
    assert set(d.blocks).isdisjoint(s.blocks)
    for i, blk in enumerate(d.blocks):
        assert torch.equal(kv.k[:, blk], before[0][i]) and torch.equal(kv.v[:, blk], before[1][i])
    kv.truncate(d, 5)
    assert len(d.blocks) == 1 and torch.equal(kv.k[:, d.blocks[0]], before[0][0])
    # the original is untouched and continues exactly as a fresh engine does
    for i, blk in enumerate(s.blocks):
        assert torch.equal(kv.k[:, blk], before[0][i]) and torch.equal(kv.v[:, blk], before[1][i])
    p2 = Prompt().add("Onderwerp: caching in de tafel, met codes.").add(t1.text, t1.ids, e.tokenizer.family).add(" Verder.")
    t2 = e.run_turns([Turn("A", p2, GREEDY)])[0]
    assert t2.metrics["reused_tokens"] == t1.metrics["prompt_tokens"] + len(t1.ids) - 1
    assert fp8_engine().run_turns([Turn("A", p2, GREEDY)])[0].ids == t2.ids


def test_cpu_engine_chunked_prefill_matches_one_shot():
    long = "woord " * 300
    a = fp8_engine(prefill_chunk=64).run_turns([Turn("K", long, GREEDY)])[0]
    b = fp8_engine(prefill_chunk=8192).run_turns([Turn("K", long, GREEDY)])[0]
    assert a.error is None and a.ids == b.ids
