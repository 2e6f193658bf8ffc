"""csrc/grammar_mask.hip on the device: the mask against ops/reference.py bit for bit (every output is an
integer decision: no tolerance), K6 on rows the mask leaves almost empty, the step hand-over of the
two-slot state inside a captured step against the CPU walker, and the engine's graph and eager paths.

Engine cases ban the vocabulary's whitespace-only tokens with ``logit_bias`` (tests/test_grammar_cpu.py
says why): with them banned the finite-language schema must finish on random weights."""
import json
import random

import pytest
import torch

from theroundtaible_amd import ops
from theroundtaible_amd.engine import Engine, EngineConfig, SamplingParams, Turn
from theroundtaible_amd.engine import grammar as G
from theroundtaible_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = G.GRAMMAR_MAX_DEPTH
BYTE_CAP = G.GRAMMAR_TOKEN_BYTE_CAP
JSON = G.compile_grammar({"type": "json_object"})
NUMBER = G.compile_grammar({"type": "regex", "pattern": r"-?\d+(\.\d+)?([eE][+-]?\d+)?"})
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


NESTING = [b"[[[", b"]]]", b'{"a":[{"b":', b"}]}", b'"}]}', b"1]]", b"[{}],", b'{"k":{"k":{"k":', b"}}}", b"]]]]]]]]",
           b"[[[[[[[[", b'":[[', b"[]]", b"{}}", b"1}]}", b'"a":[1,[2,[3]]]', b"}}", b"]}", b"[[", b'{"', b'":', b'",', b'"}',
           b"true", b"null", b"false", b"\\u", b"\\u00e9", b"\xe2\x82", b"\x82\xac", b"\xf0\x9f\x98\x80", b"0.5e+1", b"e9",
           b"  ", b"\n\t", b" :", b", "]


def synthetic_table(V: int) -> G.TokenTable:
    """Zero-byte specials (ids 0, 1, 2 and the last id; 1 and the last are stop ids), all 256 single bytes
    (V = 33: a JSON-heavy choice of them), tokens that push and pop several levels in one walk, and
    random strings of 2, 3, 17, 64, the byte cap and cap + 1 bytes: over a JSON-heavy alphabet, over
    letters (they survive inside a string to their last byte) and over digits (inside a number)."""
    rng = random.Random(V)
    pieces = [b"", b"", b""]
    if V < 300:
        pieces += [bytes([b]) for b in b'{}[]":,1 a\\u0e-.t\xc3\xa9\xe2\x82'] + NESTING
    else:
        pieces += [bytes([b]) for b in range(256)] + NESTING
    alphabets = [b'{}[]":,\\ 0123456789.-+eEtruefalsn ab\xc3\xa9', b"abcdefgh ", b"0123456789"]
    k = 0
    while len(pieces) < V:
        n = (2, 3, 17, 64, BYTE_CAP, BYTE_CAP + 1)[k % 6]
        pieces.append(bytes(rng.choice(alphabets[(k // 6) % 3]) for _ in range(n)))
        k += 1
    pieces = pieces[:V - 1] + [b""]
    return G.TokenTable(pieces, [1, V - 1], name=f"synthetic{V}")


JSON_PREFIXES = [
    ("start", b""), ("in string", b'{"a'), ("after backslash", b'{"a\\'), ("inside \\uXX", b'{"a\\u0f'),
    ("mid UTF-8", b'{"a\xe2\x82'), ("mid 4-byte UTF-8", b'{"a":"\xf0\x9f'), ("number in object", b'{"a":1'),
    ("number in array", b'{"a":[1'), ("fraction in array", b'{"a":[[0.5'), ("after a value at depth 1", b'{"a":1 '),
    ("after a key", b'{"a"'), ("literal", b'{"a":[tr'), ("depth = cap", b'{"a":' * CAP),
    ("depth = cap - 1", b'{"a":' * (CAP - 2) + b"["), ("arrays to the cap", b'{"a":' + b"[" * (CAP - 1)),
    ("done", b'{"a":[]}'),
]
NUMBER_PREFIXES = [b"", b"1", b"-", b"1.", b"12.5", b"0", b"3e", b"3e+1"]     # a number at the top level


@DTYPES
@pytest.mark.parametrize("V,pad", [(4099, 0), (4099, 5), (33, 0), (33, 7)], ids=["V4099", "V4099_ld4104", "V33", "V33_ld40"])
def test_mask_matches_the_reference_bit_for_bit(V, pad, dtype):
    table = synthetic_table(V)
    jb, nb = G.BoundGrammar(JSON, table, check=False), G.BoundGrammar(NUMBER, table, check=False)
    gm_d, gm_h = ops.GrammarMask(3, DEV, table), ops.GrammarMask(3, "cpu", table)
    g = torch.Generator().manual_seed(V)
    states = [(name, JSON.walk(JSON.start_state, p)) for name, p in JSON_PREFIXES] + [("FIN", G.FIN), ("DEAD", G.DEAD)]
    assert all(st[0] >= 0 for _, st in states[:-2])
    assert states[12][1][1] == CAP and states[13][1][1] == CAP - 1 and states[14][1][1] == CAP
    counts = []
    for k, (name, st) in enumerate(states):
        nst = NUMBER.walk(NUMBER.start_state, NUMBER_PREFIXES[k % len(NUMBER_PREFIXES)]) if k < 16 else (G.FIN, G.DEAD)[k - 16]
        rows = [(jb, st), (nb, nst), None]
        gm_d.fill(rows)
        gm_h.fill(rows)
        logits = (3.0 * torch.randn(3, V, generator=g)).to(dtype)
        logits[0, 5] = float("-inf")                        # an element that is -inf already
        buf = torch.full((3, V + pad), float("nan"), dtype=dtype, device=DEV)
        view = buf[:, :V]
        view.copy_(logits)
        assert ops.apply_grammar_mask(view, gm_d).data_ptr() == buf.data_ptr()
        want = ref.apply_grammar_mask(logits.clone(), gm_h)
        got = view.cpu()
        assert torch.equal(bits(got), bits(want)), f"{name}: the kernel and the reference differ"
        masked = torch.isinf(want.float()) & (want.float() < 0)
        assert torch.equal(bits(got)[~masked], bits(logits)[~masked]), f"{name}: an allowed element changed"
        assert torch.equal(bits(got[2]), bits(logits[2])), f"{name}: the row without a grammar changed"
        assert bool((~masked[:2]).any(dim=1).all()), f"{name}: a row without a finite element"
        if pad:
            assert bool(torch.isnan(buf[:, V:]).all()), f"{name}: wrote past column V"
        # the reference itself against the scalar walker, so the two do not share a mistake
        for i in range(V if pad == 0 else 0):
            assert bool(masked[0, i]) == (not jb.token_allowed(st, i) or i == 5), (name, i, table.pieces[i])
            assert bool(masked[1, i]) == (not nb.token_allowed(nst, i)), (name, i, table.pieces[i])
        assert gm_d.states(0) == gm_h.states(0)             # step=None: the state is only read
        counts.append(int((~masked[0]).sum()))
    print(f"ALLOWED V={V} json row per state: {counts}")
    if V > 300:
        longest = [i for i, p in enumerate(table.pieces) if len(p) == BYTE_CAP]
        over = [i for i, p in enumerate(table.pieces) if len(p) > BYTE_CAP]
        in_string = JSON.walk(JSON.start_state, b'{"a')
        assert any(jb.token_allowed(in_string, i) for i in longest) and not any(jb.token_allowed(in_string, i) for i in over)
        deep = JSON.walk(JSON.start_state, b'{"a":[')
        assert jb.token_allowed(deep, table.pieces.index(b"[[[[[[[[")) and jb.token_allowed(
            JSON.walk(deep, b"[[[[[[[["), table.pieces.index(b"]]]]]]]]"))


def test_launcher_refusals():
    table = synthetic_table(33)
    gm = ops.GrammarMask(2, DEV, table)
    with pytest.raises(ValueError, match="token table"):
        ops.apply_grammar_mask(torch.zeros(2, 34, device=DEV), gm)
    with pytest.raises(RuntimeError):
        ops.apply_grammar_mask(torch.zeros(2, 33, dtype=torch.float16, device=DEV), gm)
    with pytest.raises(RuntimeError):
        ops.apply_grammar_mask(torch.zeros(3, 33, device=DEV), gm)                 # operands cover 2 rows
    with pytest.raises(RuntimeError):
        ops.native().grammar_mask(torch.zeros(2, 33, device=DEV), gm.meta, gm.cls, gm.tab, gm.accept, gm.stops, gm.state,
                                  gm.tok_off, gm.tok_bytes, None, torch.zeros(1, dtype=torch.int64, device=DEV))


# ---- K6 on rows the mask leaves almost empty --------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("mode", ["greedy", "top_p", "top_k"])
def test_k6_samples_a_finite_element_of_a_masked_row(mode, dtype):
    """Rows with 1, 2 and 37 finite elements among V = 3 * 4096 + 123, so whole 4096-chunks are -inf:
    K6 returns a finite element's id (greedy: the largest; equal values: the lowest id)."""
    V = 3 * 4096 + 123
    g = torch.Generator().manual_seed(3)
    finite = [[V - 2], [4100, 9000], sorted(random.Random(1).sample(range(8192, V), 37))]
    logits = torch.full((3, V), float("-inf"))
    for b, ids in enumerate(finite):
        logits[b, ids] = (2.0 * torch.randn(len(ids), generator=g)).to(dtype).float()
    temp = {"greedy": 0.0}.get(mode, 1.0)
    for trial in range(6):
        got = ops.sample(logits.to(dtype).to(DEV), torch.full((3,), temp, device=DEV),
                         torch.full((3,), 0.9 if mode == "top_p" else 1.0, device=DEV),
                         torch.full((3,), 40 if mode == "top_k" else 0, dtype=torch.int32, device=DEV),
                         torch.tensor([11, 12, 13], dtype=torch.int64, device=DEV) + trial,
                         torch.full((3,), 7 + trial, dtype=torch.int64, device=DEV)).cpu().tolist()
        for b, t in enumerate(got):
            assert t in finite[b], (mode, b, t)
            if mode == "greedy":
                assert t == int(logits[b].argmax())


# ---- the captured step --------------------------------------------------------------------------------------

STEPS, CB, CV = 40, 3, 4099


@DTYPES
def test_captured_step_hands_the_state_over(dtype):
    """Capture {logits <- seq[step], grammar mask(out, step), sample_advance} once and replay it 40 times
    with no host input. After replay s the slot s & 1 holds the CPU walker's state after out[0:s]; every
    recorded id was allowed at its state; once a stop id appears only stop ids follow; a second capture
    replays the same ids. Row 0: json_object, row 1: a finite regex (it must stop), row 2: no grammar."""
    table = synthetic_table(CV)
    words = G.compile_grammar({"type": "regex", "pattern": "(ab|cd|[e-h]{3}){1,3}"})
    bounds = [G.BoundGrammar(JSON, table, check=False), G.BoundGrammar(words, table, check=False), None]
    g = torch.Generator().manual_seed(17)
    seq = (3.0 * torch.randn(STEPS, CB, CV, generator=g)).to(dtype)
    seq_d = seq.to(DEV)
    H, bs, maxb, ROWS = 64, 32, 4, 48
    embed = torch.randn(CV, H, generator=g).to(torch.bfloat16).to(DEV)
    bt = torch.arange(CB * maxb, dtype=torch.int32, device=DEV).reshape(CB, maxb)
    temp = torch.tensor([0.9, 1.0, 0.7], device=DEV)
    top_p = torch.tensor([1.0, 0.9, 1.0], device=DEV)
    top_k = torch.tensor([0, 0, 40], dtype=torch.int32, device=DEV)
    seeds = torch.tensor([5, 36, 67], dtype=torch.int64, device=DEV)
    start = [(b, b.g.start_state) if b is not None else None for b in bounds]

    def run(check_states):
        z = lambda dt: torch.zeros(CB, dtype=dt, device=DEV)                       # noqa: E731
        out = torch.zeros(ROWS, CB, dtype=torch.int64, device=DEV)
        step = torch.zeros(1, dtype=torch.int64, device=DEV)
        ids, pos, ctx, slots, offs = z(torch.int64), z(torch.int64), z(torch.int32), z(torch.int64), z(torch.int64)
        res = torch.zeros(CB, H, dtype=torch.bfloat16, device=DEV)
        logits = torch.zeros(CB, CV, dtype=dtype, device=DEV)
        nxt = z(torch.int64)
        ws = ops.sample_workspace(CB, DEV)
        gm = ops.GrammarMask(CB, DEV, table)

        def reset():
            for t in (out, step, ids, pos, slots):
                t.zero_()
            ctx.fill_(1)
            offs.fill_(1)
            gm.fill(start)

        def body():
            logits.copy_(torch.index_select(seq_d, 0, step.clamp(max=STEPS - 1))[0])
            ops.apply_grammar_mask(logits, gm, out, step)
            ops.sample_advance(logits, temp, top_p, top_k, seeds, offs, ws, nxt, out, ids, pos, ctx, step, slots, res,
                               bt, embed, bs)

        reset()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            body()                                          # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(s)
        reset()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            body()
        reset()
        states = [b.g.start_state if b is not None else None for b in bounds]
        for k in range(STEPS):
            gr.replay()
            if check_states:
                torch.cuda.synchronize()
                slot, rec = gm.states(k & 1), out[k].cpu().tolist()
                for b, bound in enumerate(bounds):
                    if bound is None:
                        continue
                    assert slot[b] == states[b], f"replay {k} row {b}: slot {k & 1} holds {slot[b]}, the walker {states[b]}"
                    assert bound.token_allowed(states[b], rec[b]), f"replay {k} row {b}: id {rec[b]} at {states[b]}"
                    states[b] = bound.advance(states[b], rec[b])
        torch.cuda.synchronize()
        assert int(step.item()) == STEPS
        return out[:STEPS].cpu()

    out = run(True)
    assert torch.equal(out, run(False)), "two captures replayed different ids"
    stops = set(table.stop_ids)
    for b in (0, 1):
        col = out[:, b].tolist()
        hit = [k for k, t in enumerate(col) if t in stops]
        if hit:
            assert set(col[hit[0]:]) <= stops, f"row {b}: a token after the stop id"
    col = out[:, 1].tolist()
    first = min(k for k, t in enumerate(col) if t in stops)
    assert 1 <= first <= 9 and words.accepts(b"".join(table.pieces[t] for t in col[:first]))
    # the row without a grammar samples what it samples without the mask launch
    plain = ops.sample(seq_d[0], temp, top_p, top_k, seeds, torch.ones(CB, dtype=torch.int64, device=DEV)).cpu()
    assert int(out[0, 2]) == int(plain[2])


# ---- engine ---------------------------------------------------------------------------------------------

PROMPT = "Geef je oordeel als JSON."
FINITE = {"type": "object", "properties": {
    "verdict": {"enum": ["yes", "no", "abstain"]}, "sure": {"type": "boolean"}, "version": {"const": 3},
    "why": {"type": "string", "maxLength": 4}}}
SPEC = {"type": "json_schema", "schema": FINITE}


def eng(**kw):
    cfg = dict(model="tiny-llama-128", weights="random-dev:3", device="cuda:0", num_blocks=512)
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


def no_padding(engine) -> dict:
    t = engine.token_table()
    ban = {i: -100.0 for i, p in enumerate(t.pieces) if p and not p.strip(b" \t\n\r")}
    assert 0 < len(ban) <= 300
    return ban


def valid(v) -> bool:
    return (isinstance(v, dict) and list(v) == ["verdict", "sure", "version", "why"] and v["verdict"] in ("yes", "no", "abstain")
            and type(v["sure"]) is bool and type(v["version"]) is int and v["version"] == 3
            and isinstance(v["why"], str) and len(v["why"]) <= 4)


@pytest.fixture(scope="module")
def engines():
    return eng(use_graphs=True), eng(use_graphs=False)


def turns(engine, extra=None, **kw):
    ban = no_padding(engine)
    mk = lambda seed, **k: SamplingParams(temperature=1.0, top_p=1.0, seed=seed, max_new_tokens=96,       # noqa: E731
                                          stop_on_consensus=False, logit_bias=dict(ban, **(extra or {})), **k, **kw)
    return [Turn("G1", PROMPT, mk(1, grammar=SPEC)), Turn("G2", PROMPT + " Kort.", mk(2, grammar=SPEC)),
            Turn("P", PROMPT, mk(3, ignore_eos=True))]


def check_replies(engine, outs, graph, eager):
    eos = engine.tokenizer.eos_id
    for a, b in zip(graph, eager):
        assert a.error is None and b.error is None
        assert a.ids == b.ids, "the graph path and the eager path sampled different ids"
    for o in outs[:2]:
        assert len(o.ids) < 70 and o.ids[-1] == eos and eos not in o.ids[:-1]
        assert valid(json.loads(o.text)), o.text
    assert len(outs[2].ids) == 96


def test_engine_graph_and_eager_paths_agree(engines):
    ge, ee = engines
    graph, eager = ge.run_turns(turns(ge)), ee.run_turns(turns(ee))
    check_replies(ge, graph, graph, eager)
    assert any("gr" in k for k in ge.graphs if isinstance(k[-1], str)), list(ge.graphs)
    # a batch without a grammar row replays the graph it replayed before the feature: no "gr" tag
    n = ge.stats["graph_captures"]
    plain = SamplingParams(temperature=0.7, seed=4, max_new_tokens=16, ignore_eos=True, stop_on_consensus=False)
    a = ge.run_turns([Turn("Q", PROMPT, plain)])[0]
    b = ee.run_turns([Turn("Q", PROMPT, plain)])[0]
    assert a.ids == b.ids and len(a.ids) == 16
    assert ge.stats["graph_captures"] == n + 1 and sum("gr" in k for k in ge.graphs if isinstance(k[-1], str)) == 1


def test_engine_with_processors_and_logprobs(engines):
    ge, ee = engines
    for e in engines:
        for key in ("G1", "G2", "P"):
            e.release(key)
    kw = dict(repetition_penalty=1.2, repeat_last_n=32, frequency_penalty=0.3, logprobs=20)
    graph, eager = ge.run_turns(turns(ge, **kw)), ee.run_turns(turns(ee, **kw))
    check_replies(ge, graph, graph, eager)
    bound = G.bind(SPEC, ge.tokenizer, int(ge.cfg.vocab))
    for o, o2 in zip(graph[:2], eager[:2]):
        st = bound.g.start_state
        assert len(o.logprobs) == len(o.ids) == len(o2.logprobs)
        for t, (lp, top_ids, top_lps), (lp2, top_ids2, _) in zip(o.ids, o.logprobs, o2.logprobs):
            assert float("-inf") < lp <= 0.0 and top_ids == top_ids2
            for i, l in zip(top_ids, top_lps):
                if l == float("-inf"):
                    assert not bound.token_allowed(st, i)
                else:
                    assert bound.token_allowed(st, i)
            st = bound.advance(st, t)
        assert st == G.FIN


def test_engine_json_object_graph_and_eager(engines):
    """json_object is no finite language: what 48 tokens give is equal on both paths, every id was allowed,
    and the text is a live prefix of a document (or a whole one)."""
    ge, ee = engines
    p = SamplingParams(temperature=1.0, seed=6, max_new_tokens=48, stop_on_consensus=False, grammar={"type": "json_object"},
                       logit_bias=no_padding(ge))
    a, b = ge.run_turns([Turn("J", PROMPT, p)])[0], ee.run_turns([Turn("J", PROMPT, p)])[0]
    assert a.error is None and a.ids == b.ids
    bound = G.bind({"type": "json_object"}, ge.tokenizer, int(ge.cfg.vocab))
    st = bound.g.start_state
    for t in a.ids:
        assert bound.token_allowed(st, t)
        st = bound.advance(st, t)
    assert JSON.live(a.text.encode("utf-8")) and (st != G.FIN or isinstance(json.loads(a.text), dict))
