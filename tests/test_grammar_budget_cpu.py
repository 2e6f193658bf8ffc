"""Budgeted grammar finish (``SamplingParams.grammar_finish``), the ``tail`` grammar and the knights'
consensus block, without a GPU: the soundness of ``need`` under two adversaries, the exact minimum
budget, the budgeted reference mask against the plain one, ``tail`` against ``re``, the all-live flags,
config, serve's 400s, and a 2-round ``discuss`` whose every reply ends in a block ``json.loads`` takes as is.

Bound used everywhere: a run started with budget ``n >= need(start) + 1`` must reach ``FIN`` within ``n``
tokens and no step may have an empty allowed set (engine/grammar.py GrammarBudget states why)."""
import itertools
import json
import random
import re
import urllib.error

import pytest
import torch

from test_grammar_cpu import FINITE, PREFIXES, PROMPT, VOCAB, _post, cpu_engine
from theroundtaible_amd import ops
from theroundtaible_amd.cli import main
from theroundtaible_amd.config import engine_settings
from theroundtaible_amd.consensus import CONSENSUS_CLOSE, CONSENSUS_OPEN, consensus_grammar, consensus_schema
from theroundtaible_amd.engine import SamplingParams, Turn
from theroundtaible_amd.engine import grammar as G
from theroundtaible_amd.engine.engine import check_budget
from theroundtaible_amd.engine.tokenizer import EngineTokenizer
from theroundtaible_amd.errors import ConfigError
from theroundtaible_amd.ops import reference as ref
from theroundtaible_amd.serve import build_server

JSON = G.compile_grammar({"type": "json_object"})
TAIL = {"type": "tail", "open": "```json\n", "body": {"type": "json_schema", "schema": FINITE}, "close": "\n```"}
REGEX = {"type": "regex", "pattern": r"(ab|c)+-?\d{2,}(\.\d+)?x*"}
DEEP = b'{"a":[[{"b":['        # json_object is driven from here: depth 5


@pytest.fixture(scope="module", autouse=True)
def one_torch_thread():
    """These tests issue thousands of small ops on vectors of V elements, right at torch's intra-op grain
    size. With one thread no op opens a parallel region: beside another busy process the spinning
    thread team made single cases take minutes. Restored when the module is done."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(threads)


@pytest.fixture(scope="module")
def tok():
    return EngineTokenizer(VOCAB)


@pytest.fixture(scope="module")
def bpe(tok):
    return G.token_table(tok, VOCAB)


@pytest.fixture(scope="module")
def synthetic():
    """A byte-level table: a stop id, every byte, and tokens that cross the seams of the grammars above."""
    pieces = [b""] + [bytes([b]) for b in range(256)] + [b'{"', b'":', b'","', b"]]", b"}]", b'"}', b"```json\n{", b"n\n", b"\n```",
                                                         b"abab", b"00", b'"why":"', b"true", b"  ", b"}\n```"]
    return G.TokenTable(pieces, [0], name="synthetic")


def bind_to(table, spec) -> G.BoundGrammar:
    return G.BoundGrammar(G.compile_grammar(spec), table)


CASES = [("finite", {"type": "json_schema", "schema": FINITE}, b""), ("json_object", {"type": "json_object"}, DEEP),
         ("regex", REGEX, b""), ("tail", TAIL, b"")]


class Walker:
    """Allowed sets of one bound pair through the vectorised reference (one walk of the whole vocabulary per
    distinct state, cached: the budget only filters it)."""

    def __init__(self, bound: G.BoundGrammar):
        self.bound, self.bd, self.V = bound, bound.budget(), bound.table.vocab
        self.gm = ops.GrammarBudgetMask(1, "cpu", bound.table).fill([(bound, bound.g.start_state, 1)])
        self.row = ref.GrammarRow(self.gm, 0)
        self.c_acc = self.gm.need[0, 0].long() & 0xFFFF
        self.c_pop = self.gm.need[1, 0].long() & 0xFFFF
        self.cache = {}

    def reference(self, st, r):
        return ref.grammar_allowed_budget(self.row, st, self.V, r, self.c_acc, self.c_pop)

    def allowed(self, st, r):
        """(ids allowed with r tokens left, need after each)."""
        if st not in self.cache:
            alive, need = self.reference(st, ref.GRAMMAR_BUDGET_FREE)
            stops = torch.zeros(self.V, dtype=torch.bool)
            stops[list(self.bound.table.stop_ids)] = True
            self.cache[st] = (alive & ~stops, alive & stops, need)
        walk, stop, need = self.cache[st]
        ok = (walk & (need <= r - 2) & (r > 0)) | stop
        return torch.nonzero(ok).squeeze(1), need


def run(w: Walker, start, budget: int, adversary: str, rng, check_every: int = 1):
    """One constrained reply under ``budget``: (ids, final state). Asserts a non-empty allowed set at every step."""
    st, ids = start, []
    for used in range(budget):
        r = budget - used
        allowed, need = w.allowed(st, r)
        assert allowed.numel() > 0, (st, r)
        if used % check_every == 0:      # the cached filter is the reference's rule
            assert torch.equal(torch.nonzero(w.reference(st, r)[0]).squeeze(1), allowed)
        if adversary == "uniform":
            t = int(allowed[rng.randrange(allowed.numel())])
        else:       # the allowed token that leaves the most still to write (a stop id leaves nothing)
            n = need[allowed].clone()
            n[torch.isin(allowed, torch.tensor(w.bound.table.stop_ids))] = -1
            t = int(allowed[int(torch.argmax(n))])
        assert w.bound.token_allowed_budget(st, t, r)
        ids.append(t)
        st = w.bound.advance(st, t)
        if st == G.FIN:
            break
    return ids, st


@pytest.mark.parametrize("name,spec,prefix", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("which", ["synthetic", "bpe"])
def test_need_is_sound_under_both_adversaries(which, name, spec, prefix, request):
    table = request.getfixturevalue(which)
    bound = bind_to(table, spec)
    w = Walker(bound)
    start = bound.g.walk(bound.g.start_state, prefix)
    assert start[0] >= 0 and (not prefix or start[1] >= 3)
    need = w.bd.need(start)
    assert 0 < need < 200
    rng = random.Random(7)
    for budget in range(need + 1, need + 41):
        for adversary in ("uniform", "greedy"):
            ids, st = run(w, start, budget, adversary, rng, check_every=1 if which == "synthetic" else 9)
            assert st == G.FIN and len(ids) <= budget, (budget, adversary, len(ids))
            assert ids[-1] in table.stop_ids and not set(ids[:-1]) & set(table.stop_ids)
            assert bound.g.accepts(prefix + b"".join(table.pieces[i] for i in ids[:-1]))
    # the exact minimum completes (the first budget above); the shortest reply takes exactly need + 1 tokens
    ids, st = run(w, start, need + 1, "greedy", rng)
    assert st == G.FIN and len(ids) == need + 1


def test_one_token_fewer_than_the_minimum_is_refused(tok, bpe):
    engine = cpu_engine()
    for spec in (c[1] for c in CASES):
        bound = G.bind(spec, tok, VOCAB)
        least = bound.budget().min_tokens()
        assert least == bound.budget().need(bound.g.start_state) + 1
        check_budget(bound, least)
        with pytest.raises(ValueError, match=f"the minimum is {least}"):
            check_budget(bound, least - 1)
        engine._prefill_turns = lambda *a, **k: (_ for _ in ()).throw(AssertionError("prefill ran"))
        p = SamplingParams(grammar=spec, grammar_finish=True, max_new_tokens=least - 1)
        for entry in (engine._run_turns_ordered, engine.start_turns):
            with pytest.raises(ValueError, match=f"the minimum is {least}"):
                entry([Turn("short", PROMPT, p)])
    with pytest.raises(ValueError, match="needs a grammar"):
        SamplingParams(grammar_finish=True).check_grammar()
    assert G.bind({"type": "json_object"}, tok, VOCAB).budget().min_tokens() == 3        # "{", "}", the stop id


def test_binding_a_budget_refuses_a_state_only_multibyte_tokens_leave():
    pieces = [b""] + [bytes([b]) for b in range(256) if b not in b"ac"] + [b"ac", b"cd"]
    table = G.TokenTable(pieces, [0], name="no-a-no-c")
    bound = bind_to(table, {"type": "regex", "pattern": "(ac)+d"})       # binds: "ac" leaves the start, "cd" the middle
    with pytest.raises(ValueError, match="only be left by multi-byte tokens"):
        bound.budget()
    assert bind_to(table, {"type": "regex", "pattern": "b+d"}).budget().min_tokens() == 3


def test_limits_agree_between_the_module_and_the_reference():
    assert (G.NEED_INF16, G.NEED_INF, G.BUDGET_FREE) == (ref.GRAMMAR_NEED_INF16, ref.GRAMMAR_NEED_INF, ref.GRAMMAR_BUDGET_FREE)
    assert G.NEED_INF > 33 * G.NEED_INF16 and G.BUDGET_FREE - 2 < G.NEED_INF


def test_need_of_json_object_counts_the_open_containers(bpe):
    bd = G.BoundGrammar(JSON, bpe).budget()
    for doc, want in ((b"", 2), (b"{", 1), (b'{"a', 4), (DEEP, 5), (DEEP + b'"x', 6), (b'{"a":' * 32, 33), (b"{}", 0)):
        assert bd.need(JSON.walk(JSON.start_state, doc)) == want, doc
    assert bd.need(G.FIN) == bd.need(G.DEAD) == 0 and sum(bd.all_live) == 0
    row_states = [JSON.walk(JSON.start_state, p) for p in PREFIXES]
    gm = ops.GrammarBudgetMask(1, "cpu", bpe).fill([(G.BoundGrammar(JSON, bpe), JSON.start_state, 9)])
    row = ref.GrammarRow(gm, 0)
    q, d, s = (torch.tensor([st[i] for st in row_states], dtype=torch.int64) for i in range(3))
    got = ref.grammar_need(row, gm.need[0, 0].long() & 0xFFFF, gm.need[1, 0].long() & 0xFFFF, q, d, s)
    assert got.tolist() == [bd.need(st) for st in row_states]


def test_a_budget_that_binds_nothing_is_the_plain_mask_bit_for_bit(tok, bpe):
    """At every state the plain reference's own bit-for-bit test visits: rows without ``grammar_finish`` in
    the budgeted launch, and a finishing row whose budget is far above every need."""
    bound = G.bind({"type": "json_object"}, tok, VOCAB)
    rx = G.bind({"type": "regex", "pattern": r"-?\d+(\.\d+)?"}, tok, VOCAB)
    plain = ops.GrammarMask(3, "cpu", bpe)
    budgeted = ops.GrammarBudgetMask(3, "cpu", bpe)
    states = [JSON.walk(JSON.start_state, p) for p in PREFIXES] + [G.FIN, G.DEAD]
    for st in states:
        logits = torch.randn(3, VOCAB + 5)[:, :VOCAB]
        want = ops.apply_grammar_mask(logits.clone(), plain.fill([(bound, st), None, (rx, rx.g.start_state)]))
        for left in (None, 4000):
            got = ops.apply_grammar_mask_budget(logits.clone(), budgeted.fill([(bound, st, left), None,
                                                                               (rx, rx.g.start_state, left)]))
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (st, left)
        assert torch.equal(want[1], logits[1])
    # a binding budget differs, and only by removing tokens
    st = JSON.walk(JSON.start_state, b'{"a":[')
    want = ops.apply_grammar_mask(torch.zeros(1, VOCAB), ops.GrammarMask(1, "cpu", bpe).fill([(bound, st)]))
    got = ops.apply_grammar_mask_budget(torch.zeros(1, VOCAB), ops.GrammarBudgetMask(1, "cpu", bpe).fill([(bound, st, 3)]))
    fw, fg = torch.isfinite(want[0]), torch.isfinite(got[0])
    assert bool((fw | ~fg).all()) and 0 < int(fg.sum()) < int(fw.sum())
    assert bool(fg[bpe.pieces.index(b"]")]) and not bool(fg[bpe.pieces.index(b"[")]) and not bool(fg[bpe.pieces.index(b"1")])
    for left in (0, -1):      # an exhausted budget: stop ids only
        got = ops.apply_grammar_mask_budget(torch.zeros(1, VOCAB), ops.GrammarBudgetMask(1, "cpu", bpe).fill([(bound, st, left)]))
        assert torch.nonzero(torch.isfinite(got[0])).squeeze(1).tolist() == list(bpe.stop_ids)


def test_reference_graph_form_hands_over_state_and_budget(tok, bpe):
    """r = budget - step: the captured form of a run with the exact minimum ends at that step."""
    bound = G.bind({"type": "json_object"}, tok, VOCAB)
    st = JSON.walk(JSON.start_state, b'{"k":[[')
    budget = bound.budget().need(st) + 1
    gm = ops.GrammarBudgetMask(2, "cpu", bpe).fill([(bound, st, budget), None])
    out = torch.zeros(budget + 2, 2, dtype=torch.int64)
    step = torch.zeros(1, dtype=torch.int64)
    ids = []
    for s in range(budget + 1):
        logits = torch.zeros(2, VOCAB)
        ops.apply_grammar_mask_budget(logits, gm, out, step)
        assert bool(torch.isfinite(logits[1]).all())
        allowed = torch.nonzero(torch.isfinite(logits[0])).squeeze(1).tolist()
        assert allowed == [i for i in allowed if bound.token_allowed_budget(st, i, budget - s)] and allowed
        t = max(allowed, key=lambda i: (bound.budget().need(bound.advance(st, i)), i))
        ids.append(t)
        out[s, 0] = t
        step += 1
        st = bound.advance(st, t)
    assert ids[budget - 1] in bpe.stop_ids and ids[budget] in bpe.stop_ids and not set(ids[:budget - 1]) & set(bpe.stop_ids)
    assert gm.states(budget & 1)[0] == G.FIN or gm.states((budget - 1) & 1)[0] == G.FIN


# ---- tail ---------------------------------------------------------------------------------------------------

def tail_accepts(opener: bytes, body: str, close: bytes, data: bytes) -> bool:
    at = data.find(opener)
    return at >= 0 and re.fullmatch(body.encode() + re.escape(close), data[at + len(opener):], re.S) is not None


@pytest.mark.parametrize("opener,body,close", [("aab", "x+", "!"), ("abab", "(a|bx)*", ""), ("aa", "[ab]x?", "aa")])
def test_tail_agrees_with_re_where_the_opener_overlaps_itself(opener, body, close):
    g = G.compile_grammar({"type": "tail", "open": opener, "body": {"type": "regex", "pattern": body}, "close": close})
    assert not g.uses_stack and not g.accept[g.start]
    n = 0
    for length in range(0, 9):
        for chars in itertools.product(b"abx!", repeat=length):
            data = bytes(chars)
            assert g.accepts(data) == tail_accepts(opener.encode(), body, close.encode(), data), data
            n += 1
    assert n > 80000
    # the free states are total on all 256 bytes and accept nothing: no stop id before the block
    for prefix in (b"", b"a", b"\x00\xff{}", opener.encode()[:-1]):
        st = g.walk(g.start_state, prefix)
        assert st[0] >= 0 and not g.is_accepting(st)
        assert all(g.walk(st, bytes([b]))[0] >= 0 for b in range(256)) or prefix == opener.encode()[:-1]


def test_tail_tokens_that_straddle_the_seam(synthetic):
    bound = bind_to(synthetic, TAIL)
    g = bound.g
    p = synthetic.pieces.index
    text = [b"o", b"k", b"`", b"`", b"```json\n{", b'"', b"v", b"e"]
    st = bound.state_after([p(x) for x in text])
    assert st == g.walk(g.start_state, b"".join(text)) and st[0] >= 0
    free = g.walk(g.start_state, b"text ```jso")
    assert bound.token_allowed(free, p(b"n\n")) and bound.token_allowed(free, p(b"n")) and bound.token_allowed(free, p(b"}\n```"))
    almost = g.walk(g.start_state, b"```json")
    assert bound.token_allowed(almost, p(b"\n")) and not bound.token_allowed(g.walk(almost, b"\n"), p(b"x"))
    assert bound.token_allowed(g.walk(g.start_state, b"``"), p(b"```json\n{"))      # "`````json\n{": still one opener
    doc = b'free ``` text ```json\n{"verdict":"no","sure":true,"version":3,"why":"x"}\n```'
    assert g.accepts(doc) and not g.accepts(doc + b"\n") and not g.accepts(doc[:-1])
    end = g.walk(g.start_state, doc[:-5])
    assert bound.token_allowed(end, p(b"}\n```")) and g.is_accepting(g.walk(end, b"}\n```"))
    with pytest.raises(ValueError, match="json_schema or regex"):
        G.compile_grammar({"type": "tail", "open": "x", "body": {"type": "json_object"}, "close": ""})
    for bad in ({"open": ""}, {"open": "x" * 33}, {"close": "y" * 33}, {"open": 3}):
        with pytest.raises(ValueError, match="tail grammar"):
            G.compile_grammar({**TAIL, **bad})


def test_a_planted_vocabulary_clears_the_all_live_flag():
    spec = {"type": "tail", "open": "ab", "body": {"type": "regex", "pattern": "x+"}, "close": ""}
    g = G.compile_grammar(spec)
    s0, s1, body = (g.walk(g.start_state, d)[0] for d in (b"", b"a", b"ab"))
    single = [b""] + [bytes([b]) for b in range(256)]

    def flags(extra):
        return G.BoundGrammar(g, G.TokenTable(single + extra, [0])).all_live()

    assert [i for i, f in enumerate(flags([])) if f] == sorted({s0, s1})          # bytes alone never die in free text
    assert [i for i, f in enumerate(flags([b"bx", b"abx", b"zab"])) if f] == sorted({s0, s1})
    assert [i for i, f in enumerate(flags([b"bq"])) if f] == [s0]                 # from "a": "b" opens, "q" is no body
    assert [i for i, f in enumerate(flags([b"abq"])) if f] == []                  # the whole opener plus a bad byte
    assert not flags([])[body]
    bd = G.BoundGrammar(g, G.TokenTable(single + [b"bq"], [0])).budget()
    assert bd.need_cap == 3 == bd.need(g.start_state) and bd.need((body, 0, 0)) == 1


# ---- config, knights ------------------------------------------------------------------------------------------

def knights_config(engine=None, per_knight=None):
    from theroundtaible_amd.types import RoundtableConfig
    per_knight = per_knight or [{}, {}]
    return RoundtableConfig.from_dict({
        "version": "1.0", "project": "cg", "language": "nl",
        "knights": [{"name": f"Ridder{i}", "adapter": f"local-llm-r{i}", "capabilities": ["x"], "priority": i + 1}
                    for i in range(len(per_knight))],
        "rules": {"max_rounds": 1, "consensus_threshold": 9, "timeout_per_turn_seconds": 300, "escalate_to_user_after": 5,
                  "auto_execute": False, "ignore": [".git"], "round_mode": "parallel"},
        "chronicle": ".roundtable/chronicle.md",
        "engine": {"default_model": "tiny-llama", "device": "cpu", "max_new_tokens": 160, **(engine or {})},
        "adapter_config": {f"local-llm-r{i}": {"engine": e} for i, e in enumerate(per_knight)}})


def test_config_field_override_and_refusal():
    from theroundtaible_amd.knights.base import TurnRequest
    from theroundtaible_amd.knights.registry import BackendFactory
    assert engine_settings(knights_config(), "local-llm-r0")["consensus_grammar"] is False
    cfg = knights_config({"consensus_grammar": True}, [{}, {"consensus_grammar": False}])
    assert [engine_settings(cfg, f"local-llm-r{i}")["consensus_grammar"] for i in range(2)] == [True, False]
    for bad in (knights_config({"consensus_grammar": True, "scripted_consensus": {"free_tokens": 4}}),
                knights_config({"scripted_consensus": {"free_tokens": 4}}, [{"consensus_grammar": True}, {}]),
                knights_config({"consensus_grammar": "yes"})):
        with pytest.raises(ConfigError, match="consensus_grammar"):
            engine_settings(bad, "local-llm-r0")
    factory = BackendFactory(cfg)
    on, off = (factory.create(f"local-llm-r{i}") for i in range(2))
    turn = on._turn(TurnRequest("t/Ridder0", PROMPT, 1, None, consensus=True), 5.0)
    assert turn.params.grammar == consensus_grammar() and turn.params.grammar_finish and not turn.params.stop_on_consensus
    for backend, req in ((on, TurnRequest("apply:Ridder0", PROMPT, 0, 64)), (off, TurnRequest("t/Ridder1", PROMPT, 1, None, consensus=True))):
        assert backend._turn(req, 5.0).params.grammar is None      # apply / code-red turns, and the knight that opted out
    schema = consensus_schema()
    assert list(schema["properties"]) == ["consensus_score", "agrees_with", "pending_issues", "files_to_modify",
                                          "file_requests", "verify_commands"]
    assert schema["properties"]["file_requests"]["maxItems"] == schema["properties"]["verify_commands"]["maxItems"] == 4
    example = json.load(open(__file__.replace("tests/test_grammar_budget_cpu.py", "examples/config.consensus-grammar.json")))
    assert example["engine"]["consensus_grammar"] is True


def test_discuss_with_consensus_grammar_always_yields_a_parseable_block(project):
    """Tiny random weights, no script: two rounds, every reply of every knight is free text and then a
    fenced block that ``json.loads`` takes as it stands (no ``repair_json``), inside max_new_tokens."""
    assert main(["--quiet", "init", "--yes", "--model", "tiny-llama", "--knights", "2", "--max-new-tokens", "150"]) == 0
    path = project / ".roundtable" / "config.json"
    cfg = json.load(open(path))
    cfg["rules"].update(max_rounds=2, round_mode="parallel")
    cfg["engine"].update(consensus_grammar=True, temperature=1.0)
    json.dump(cfg, open(path, "w"))
    assert main(["--quiet", "discuss", "Hoe sluiten we elk antwoord af?", "--no-read-codebase", "--choice", "0",
                 "--device", "cpu", "--seed", "1"]) == 0
    sp = project / ".roundtable" / "sessions"
    sp = sp / [d for d in sp.iterdir()][0].name
    rounds = [json.loads(l) for l in open(sp / "rounds.jsonl")]
    assert len(rounds) == 4 and {r["round"] for r in rounds} == {1, 2}
    keys = list(consensus_schema()["properties"])
    for r in rounds:
        text = r["response"]
        at = text.index(CONSENSUS_OPEN)
        assert text.endswith(CONSENSUS_CLOSE)
        block = json.loads(text[at + len(CONSENSUS_OPEN):-len(CONSENSUS_CLOSE)])
        assert list(block) == keys and block["consensus_score"] in range(11)
        assert all(isinstance(block[k], list) and all(isinstance(x, str) for x in block[k]) for k in keys[1:])
        assert r["consensus"] is not None and r["consensus"]["consensus_score"] == block["consensus_score"]
    decoded = [m["decode_tokens"] for m in map(json.loads, filter(str.strip, open(sp / "metrics.jsonl"))) if "knight" in m]
    assert len(decoded) == 4 and all(0 < n <= 150 for n in decoded)


# ---- serve --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def server():
    srv = build_server("tiny-llama", weights="random:1", device="cpu", port=0, max_batch=4, max_tokens=96,
                       num_blocks=512).start()
    yield srv
    srv.close()


SCHEMA_RF = {"type": "json_schema", "json_schema": {"schema": FINITE}}
BAD = [("no grammar", {"guided_finish": True}, "needs a grammar"),
       ("not a bool", {"guided_finish": "yes", "response_format": {"type": "json_object"}}, "guided_finish"),
       ("max_tokens too small", {"guided_finish": True, "response_format": SCHEMA_RF, "max_tokens": 20}, "the minimum is "),
       ("json_object below 3", {"guided_finish": True, "response_format": {"type": "json_object"}, "max_tokens": 2}, "the minimum is 3"),
       ("tail is not exposed", {"guided_finish": True, "response_format": {"type": "tail"}}, "response_format")]


@pytest.mark.parametrize("name,extra,message", BAD, ids=[b[0] for b in BAD])
def test_serve_guided_finish_400s(server, name, extra, message):
    for path, body in (("/v1/completions", {"prompt": "x", "max_tokens": 8}),
                       ("/v1/chat/completions", {"messages": [{"role": "user", "content": "x"}], "max_tokens": 8})):
        with pytest.raises(urllib.error.HTTPError) as ei:
            _post(server.url + path, {**body, **extra})
        assert ei.value.code == 400
        err = json.loads(ei.value.read().decode())["error"]
        assert err["type"] == "invalid_request_error" and message in err["message"], err


def test_serve_guided_finish_always_parses(server):
    """No whitespace ban, temperature 1, random weights: the document closes inside max_tokens and the
    request finishes with "stop", over the chunked decode of the scheduler."""
    for n, rf in ((24, {"type": "json_object"}), (60, SCHEMA_RF)):
        for seed in (1, 2):
            code, raw = _post(server.url + "/v1/completions", {"prompt": PROMPT, "max_tokens": n, "temperature": 1.0, "seed": seed,
                                                               "response_format": rf, "guided_finish": True})
            out = json.loads(raw)
            assert code == 200 and out["choices"][0]["finish_reason"] == "stop", out
            assert isinstance(json.loads(out["choices"][0]["text"]), dict) and out["usage"]["completion_tokens"] <= n
