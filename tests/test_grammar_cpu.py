"""Grammar-constrained decoding on the CPU: the byte-level automata against independent oracles
(``json.loads``, ``re.fullmatch``, a schema validator written here), the token byte table, the pairing
check, the reference mask against the scalar walker, and the feature through the CPU engine and serve.

Engine and serve cases ban the vocabulary's whitespace-only tokens with ``logit_bias``: the grammars
allow unbounded whitespace between JSON tokens (a model may pad; ``max_tokens`` bounds it), and a
random-weight model pads. With those tokens banned every token consumes at least one byte of the
finite language, so random logits must finish."""
import itertools
import json
import random
import re
import urllib.error
import urllib.request

import pytest
import torch

from theroundtaible_amd import ops
from theroundtaible_amd.engine import Engine, EngineConfig, SamplingParams, Turn
from theroundtaible_amd.engine import grammar as G
from theroundtaible_amd.engine.tokenizer import EngineTokenizer, _fallback_piece
from theroundtaible_amd.ops import reference as ref
from theroundtaible_amd.serve import build_server

JSON = G.compile_grammar({"type": "json_object"})
CAP = G.GRAMMAR_MAX_DEPTH


def loads_dict(data: bytes) -> bool:
    """The oracle: well-formed UTF-8 (strict: ``json.loads`` on bytes would let encoded surrogates
    pass) that ``json.loads`` turns into a dict, with nothing after the closing brace."""
    try:
        text = data.decode("utf-8")
        return isinstance(json.loads(text), dict) and text.endswith("}")
    except (ValueError, RecursionError):
        return False


# ---- json_object ----------------------------------------------------------------------------------------

def test_json_every_short_string_agrees_with_json_loads():
    n = 0
    for length in range(7):
        for tup in itertools.product(b'{}[]":,1', repeat=length):
            data = bytes(tup)
            n += 1
            ok = JSON.accepts(data)
            assert ok == loads_dict(data), data
            if ok:
                assert all(JSON.live(data[:i]) for i in range(len(data)))
    assert n == sum(8 ** i for i in range(7))


VALID = [
    b'{}', b' \t\n\r{ }', b'{"a":1}', b'{ "a" : 1 , "b" : [ ] }',
    b'{"esc":"\\" \\\\ \\/ \\b \\f \\n \\r \\t"}',
    b'{"u":"\\u00e9\\u20AC\\ud83d\\ude00\\uD800"}',
    '{"utf8":"é € 😀 ߿ ࠀ ￿ \U00010000 \U0010ffff \x7f"}'.encode("utf-8"),
    '{"é":"ключ"}'.encode("utf-8"),
    b'{"n":[0,-0,1,-1,10,123456789012345678901234567890,0.5,-0.5,1.25e10,1E10,1e+10,1e-10,0e0,-0.0E-0,9.9E+99]}',
    b'{"l":[true,false,null],"o":{"p":{"q":[[],[[]],{}]}}}',
    b'{"a":[1,2,{"b":"c"}],"a":null}',
    b'{"":""}', b'{"a":\n[\n1\n,\n2\n]\n}',
]
INVALID = [
    b'', b'[]', b'1', b'"a"', b'{} ', b'{}{}', b'{"a":1}x', b'{a:1}', b"{'a':1}", b'{"a":1,}', b'{"a"}', b'{"a":}',
    b'{"a":[1,]}', b'{"a":[,1]}', b'{"a":01}', b'{"a":1.}', b'{"a":-}', b'{"a":+1}', b'{"a":.5}', b'{"a":1e}',
    b'{"a":1e+}', b'{"a":00}', b'{"a":-01}', b'{"a":0x1}', b'{"a":tru}', b'{"a":True}', b'{"a":nul}',
    b'{"a":"\\x"}', b'{"a":"\\u12"}', b'{"a":"\\u12G4"}', b'{"a":"\n"}', b'{"a":"\t"}', b'{"a":"\x00"}',
    b'{"a":"\xc0\x80"}', b'{"a":"\xc1\xbf"}', b'{"a":"\xe0\x80\x80"}', b'{"a":"\xe0\x9f\xbf"}', b'{"a":"\xf0\x80\x80\x80"}',
    b'{"a":"\xf0\x8f\xbf\xbf"}', b'{"a":"\xed\xa0\x80"}', b'{"a":"\xed\xbf\xbf"}', b'{"a":"\xf4\x90\x80\x80"}',
    b'{"a":"\xf5\x80\x80\x80"}', b'{"a":"\xc3"}', b'{"a":"\xe2\x82"}', b'{"a":"\xf0\x9f\x98"}', b'{"a":"\x80"}',
    b'{"a":"\xc3\x28"}', b'{"a":"\xff"}', b'{"a":1]', b'{"a":[1}', b'{"a":[1}]',
]


def test_json_corpus():
    for doc in VALID:
        assert loads_dict(doc) and JSON.accepts(doc), doc
        assert all(JSON.live(doc[:i]) for i in range(len(doc) + 1)), doc
    for doc in INVALID:
        assert not loads_dict(doc) and not JSON.accepts(doc), doc


def test_json_depth_cap():
    open_, close = b'{"a":' * CAP, b'}' * CAP
    at_cap = open_ + b'1' + close
    assert loads_dict(at_cap) and JSON.accepts(at_cap)
    assert all(JSON.live(at_cap[:i]) for i in range(len(at_cap)))
    st = JSON.walk(JSON.start_state, open_)
    assert st[1] == CAP and st[2] == 0
    assert JSON.walk(st, b"{") == G.DEAD and JSON.walk(st, b"[") == G.DEAD        # dead at the push
    assert not JSON.accepts(b'{"a":' * (CAP + 1) + b'1' + b'}' * (CAP + 1))
    arrays = b'{"a":' + b'[' * (CAP - 1) + b']' * (CAP - 1) + b'}'
    assert JSON.accepts(arrays)
    st = JSON.walk(JSON.start_state, b'{"a":' + b'[' * (CAP - 1))
    assert st[1] == CAP and st[2] == (1 << CAP) - 2                               # bit i = container i, 1 = array
    assert JSON.walk(JSON.start_state, b"}") == G.DEAD                            # a pop on the empty stack


def test_json_single_byte_mutations_agree_with_json_loads():
    rng = random.Random(11)
    pool = b'{}[]":,\\/ \t\n\r0123456789.-+eEtrufalsn\x00\x1f\x7f\x80\xbf\xc2\xc3\xe0\xed\xf0\xf4\xffabAF'
    n = flipped = 0
    for doc in VALID:
        for _ in range(40):
            i = rng.randrange(len(doc))
            mut = doc[:i] + bytes([rng.choice(pool)]) + doc[i + 1:]
            want = loads_dict(mut)
            assert JSON.accepts(mut) == want, mut
            n += 1
            flipped += not want
    assert n >= 200 and 50 < flipped < n


# ---- regex ------------------------------------------------------------------------------------------------

PATTERNS = [r"a(b|c)*d", r"[a-c]{2,4}x?", r"\d+(\.\d+)?", r"(ab|a)(c|bc)d*", r"[^ab]c.", r"(a|b)*abb", r"a{3}", r"a{2,}b",
            r"(?:ab){1,2}|c+", r"\w\s\d", r"\W\S\D", r"[\d.]+x", r"[a\-c]+", r"[]a]+", r"a\.b\|c", r"(|a)b", r"x(a|b|cd)?x",
            r"[^\d\s]{1,3}", r"(a*b*)*c", r"\x61\t?b", r"-?(0|[1-9]\d*)", r"(yes|no|maybe)( (yes|no)){0,2}"]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_regex_agrees_with_re_fullmatch(pattern):
    g = G.compile_grammar({"type": "regex", "pattern": pattern})
    assert not g.uses_stack
    rx = re.compile(pattern.encode())
    rng = random.Random(pattern)
    alphabet = "abcdx.1 9-|]\ty"
    seen = 0
    for _ in range(4000):
        s = "".join(rng.choice(alphabet) for _ in range(rng.randint(0, 8))).encode()
        want = rx.fullmatch(s) is not None
        assert g.accepts(s) == want, (pattern, s)
        seen += want
    for s in (b"", b"a", b"ab", b"abb", b"aaa", b"abd", b"acd", b"yes no", b"12.5", b"-10", b"xcdx"):
        assert g.accepts(s) == (rx.fullmatch(s) is not None), (pattern, s)


def test_regex_utf8():
    g = G.compile_grammar({"type": "regex", "pattern": "é+[α-ω]x"})
    assert g.accepts("ééβx".encode()) and not g.accepts("éx".encode()) and not g.accepts("é".encode()[:1] + b"x")
    dot = G.compile_grammar({"type": "regex", "pattern": "a.b"})
    for ch in ("x", "é", "€", "😀"):
        assert dot.accepts(f"a{ch}b".encode())
    assert not dot.accepts(b"a\nb") and not dot.accepts(b"a\xc3b") and not dot.accepts(b"a\xed\xa0\x80b")
    neg = G.compile_grammar({"type": "regex", "pattern": "[^a-y€]+"})
    assert neg.accepts("zé😀\n".encode()) and not neg.accepts("€".encode()) and not neg.accepts(b"b")
    assert not neg.accepts(b"\xff") and not neg.accepts(b"\xc0\x80")


@pytest.mark.parametrize("pattern", ["(a", "a)", "a**?", "a+?", "*a", "[a", "a{2,1}", "^a", "a$", r"\1", r"(?=a)b", r"\p{L}",
                                     "a{99999}", r"\b"])
def test_regex_refusals(pattern):
    with pytest.raises(ValueError, match="regex"):
        G.compile_grammar({"type": "regex", "pattern": pattern})


# ---- json_schema ------------------------------------------------------------------------------------------

SCHEMA = {"type": "object", "properties": {
    "verdict": {"enum": ["yes", "no", "abstain"]},
    "sure": {"type": "boolean"},
    "version": {"const": 3},
    "why": {"type": "string", "minLength": 1, "maxLength": 6},
    "scores": {"type": "array", "items": {"type": "integer"}, "minItems": 1, "maxItems": 3},
    "extra": {"anyOf": [{"type": "null"}, {"type": "number"},
                        {"type": "object", "properties": {"tag": {"type": "string", "enum": ["a", "b"]}}}]},
    "none": {"type": "array", "items": {"type": "boolean"}, "maxItems": 0},
}, "required": ["verdict", "sure", "version", "why", "scores", "extra", "none"], "additionalProperties": False}


def validate(schema, v) -> bool:
    """The schema subset's meaning, written independently of the compiler."""
    if "anyOf" in schema:
        return any(validate(s, v) for s in schema["anyOf"])
    if "const" in schema:
        return type(v) is type(schema["const"]) and v == schema["const"]
    if "enum" in schema:
        return any(type(v) is type(e) and v == e for e in schema["enum"])
    t = schema["type"]
    if t == "object":
        props = schema.get("properties", {})
        return isinstance(v, dict) and list(v) == list(props) and all(validate(props[k], v[k]) for k in props)
    if t == "array":
        return (isinstance(v, list) and schema.get("minItems", 0) <= len(v) <= schema.get("maxItems", 1 << 30)
                and all(validate(schema["items"], x) for x in v))
    if t == "string":
        return isinstance(v, str) and schema.get("minLength", 0) <= len(v) <= schema.get("maxLength", 1 << 30)
    if t == "integer":
        return type(v) is int
    if t == "number":
        return type(v) in (int, float)
    if t == "boolean":
        return type(v) is bool
    return t == "null" and v is None


def instance(schema, rng):
    if "anyOf" in schema:
        return instance(rng.choice(schema["anyOf"]), rng)
    if "const" in schema:
        return schema["const"]
    if "enum" in schema:
        return rng.choice(schema["enum"])
    t = schema["type"]
    if t == "object":
        return {k: instance(s, rng) for k, s in schema.get("properties", {}).items()}
    if t == "array":
        n = rng.randint(schema.get("minItems", 0), schema.get("maxItems", schema.get("minItems", 0) + 2))
        return [instance(schema["items"], rng) for _ in range(n)]
    if t == "string":
        n = rng.randint(schema.get("minLength", 0), schema.get("maxLength", 5))
        return "".join(rng.choice(['a', 'Z', ' ', 'é', '€', '😀', '"', '\\', '\n', '/']) for _ in range(n))
    if t == "integer":
        return rng.choice([0, 7, -12, 10 ** 12])
    if t == "number":
        return rng.choice([0, -3, 2.5, 1e-7, -1.5e22])
    return rng.choice([True, False]) if t == "boolean" else None


def dumps(v, rng) -> bytes:
    sep = rng.choice([(",", ":"), (", ", ": "), (" ,\n", " :\t")])
    return json.dumps(v, ensure_ascii=rng.random() < 0.5, separators=sep).encode("utf-8")


def test_schema_instances_accept_and_wrong_ones_reject():
    g = G.compile_grammar({"type": "json_schema", "schema": SCHEMA})
    assert not g.uses_stack
    rng = random.Random(5)
    for _ in range(300):
        v = instance(SCHEMA, rng)
        assert validate(SCHEMA, v)
        doc = dumps(v, rng)
        assert g.accepts(doc), doc
        assert all(g.live(doc[:i]) for i in range(len(doc)))
    good = instance(SCHEMA, rng)
    wrong = [dict(good, verdict="perhaps"), dict(good, verdict=1), dict(good, sure="true"), dict(good, version=4),
             dict(good, version="3"), dict(good, why=""), dict(good, why="1234567"), dict(good, why="€" * 7),
             dict(good, scores=[]), dict(good, scores=[1, 2, 3, 4]), dict(good, scores=[1.5]), dict(good, extra="x"),
             dict(good, extra={"tag": "c"}), dict(good, none=[True]), {k: v for k, v in good.items() if k != "why"},
             dict(good, more=1), dict(reversed(list(good.items())))]
    for v in wrong:
        assert not validate(SCHEMA, v)
        assert not g.accepts(json.dumps(v).encode()), v
    assert g.accepts(json.dumps(dict(good, why="€" * 6), ensure_ascii=False).encode())
    assert g.accepts(json.dumps(dict(good, why="€" * 6), ensure_ascii=True).encode())     # \\uXXXX counts once


UNSUPPORTED = [
    ("$ref", {"$ref": "#/definitions/x"}), ("pattern", {"type": "string", "pattern": "a+"}),
    ("additionalProperties", {"type": "object", "properties": {}, "additionalProperties": True}),
    ("minimum", {"type": "integer", "minimum": 0}), ("maximum", {"type": "number", "maximum": 1}),
    ("exclusiveMinimum", {"type": "number", "exclusiveMinimum": 0}), ("multipleOf", {"type": "integer", "multipleOf": 2}),
    ("format", {"type": "string", "format": "date"}), ("oneOf", {"oneOf": [{"type": "null"}]}),
    ("allOf", {"allOf": [{"type": "null"}]}), ("not", {"not": {"type": "null"}}),
    ("patternProperties", {"type": "object", "patternProperties": {"a": {"type": "null"}}}),
    ("uniqueItems", {"type": "array", "items": {"type": "null"}, "uniqueItems": True}),
    ("prefixItems", {"type": "array", "prefixItems": [{"type": "null"}]}),
    ("minProperties", {"type": "object", "properties": {}, "minProperties": 1}),
    ("required", {"type": "object", "properties": {"a": {"type": "null"}, "b": {"type": "null"}}, "required": ["a"]}),
    ("if", {"if": {"type": "null"}}), ("definitions", {"type": "null", "definitions": {}}),
]


@pytest.mark.parametrize("keyword,schema", UNSUPPORTED, ids=[u[0] for u in UNSUPPORTED])
def test_schema_unsupported_keywords_raise(keyword, schema):
    with pytest.raises(ValueError, match=re.escape(keyword)):
        G.compile_grammar({"type": "json_schema", "schema": {"type": "object", "properties": {"x": schema}}})


def test_caps_and_bad_specs_raise():
    with pytest.raises(ValueError, match="states"):
        G.compile_grammar({"type": "json_schema", "schema": {"type": "array", "items": {"type": "string", "maxLength": 40},
                                                             "maxItems": 40}})
    with pytest.raises(ValueError, match="classes"):
        chars = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ_-,;:=@#%&"       # 72, one class each
        G.compile_grammar({"type": "regex", "pattern": "".join(f"(?:{re.escape(c)}{{{i + 1}}})?" for i, c in enumerate(chars))})
    for bad in (None, "json", {}, {"type": "yaml"}, {"type": "regex"}, {"type": "json_object", "schema": {}},
                {"type": "json_schema", "schema": {"type": "object"}, "strict": True}):
        with pytest.raises(ValueError):
            G.compile_grammar(bad)
    p = SamplingParams(grammar={"type": "json_object"}, ignore_eos=True)
    assert p.wants_grammar() and not SamplingParams().wants_grammar()
    with pytest.raises(ValueError, match="ignore_eos"):
        p.check_grammar()
    with pytest.raises(ValueError, match="pattern"):
        SamplingParams(grammar={"type": "json_schema", "schema": {"type": "string", "pattern": "a"}}).check_grammar()
    SamplingParams(grammar={"type": "json_object"}).check_grammar()
    SamplingParams().check_grammar()
    assert G.compile_grammar({"type": "json_object"}) is JSON                     # cached by the canonical spec


def test_every_state_of_every_grammar_reaches_accept():
    grammars = [JSON, G.compile_grammar({"type": "json_schema", "schema": SCHEMA})]
    grammars += [G.compile_grammar({"type": "regex", "pattern": p}) for p in PATTERNS]
    for g in grammars:
        assert all(g.reaches_accept()), g.key
        assert g.n_states <= G.GRAMMAR_MAX_STATES and g.n_classes <= G.GRAMMAR_MAX_CLASSES
        assert len(g.trans) == g.n_states * g.n_classes <= G.GRAMMAR_MAX_TABLE
        assert all(e == G.DEAD_ENTRY or (e >> 2) < g.n_states for e in g.trans)


def test_limits_agree_between_the_module_and_the_reference():
    assert (G.GRAMMAR_MAX_DEPTH, G.GRAMMAR_MAX_STATES, G.GRAMMAR_MAX_CLASSES, G.GRAMMAR_MAX_TABLE, G.GRAMMAR_TOKEN_BYTE_CAP,
            G.GRAMMAR_MAX_STOPS, G.Q_FIN, G.Q_DEAD) == \
        (ref.GRAMMAR_MAX_DEPTH, ref.GRAMMAR_MAX_STATES, ref.GRAMMAR_MAX_CLASSES, ref.GRAMMAR_MAX_TABLE,
         ref.GRAMMAR_TOKEN_BYTE_CAP, ref.GRAMMAR_MAX_STOPS, ref.GRAMMAR_Q_FIN, ref.GRAMMAR_Q_DEAD)
    if ops.native_available():
        assert list(ops.native().GRAMMAR_LIMITS)[:6] == [G.GRAMMAR_MAX_DEPTH, G.GRAMMAR_MAX_STATES, G.GRAMMAR_MAX_CLASSES,
                                                         G.GRAMMAR_MAX_TABLE, G.GRAMMAR_TOKEN_BYTE_CAP, G.GRAMMAR_MAX_STOPS]


# ---- token table, binding -----------------------------------------------------------------------------------

VOCAB = 32768 + 40      # the BPE's 32000 ids plus fallback ids


@pytest.fixture(scope="module")
def tok():
    return EngineTokenizer(VOCAB)


@pytest.fixture(scope="module")
def table(tok):
    return G.token_table(tok, VOCAB)


def test_token_table_round_trips_through_decode(tok, table):
    assert table.vocab == VOCAB and G.token_table(tok, VOCAB) is table
    checked = 0
    for i in range(tok.base_vocab):
        try:
            text = table.pieces[i].decode("utf-8")
        except UnicodeDecodeError:
            continue
        if i in (tok.bos_id, tok.eos_id) or not text:
            continue
        assert tok.decode([i]) == text, i
        checked += 1
    assert checked > 30000
    for i in range(tok.base_vocab, VOCAB):
        assert table.pieces[i] == _fallback_piece(i).encode() == tok.decode([i]).encode()
    assert {bytes([b]) for b in range(256)} <= set(table.pieces)                  # byte-level: every byte is a token
    off, data = table.tensors("cpu")
    assert off.dtype == torch.int32 and off.numel() == VOCAB + 1 and data.dtype == torch.uint8
    assert int(off[-1]) == sum(len(p) for p in table.pieces) <= data.numel() < int(off[-1]) + 17 and data.numel() % 16 == 0
    i = table.pieces.index(b'{"')
    assert bytes(data[int(off[i]):int(off[i + 1])].tolist()) == b'{"'


def test_stop_ids_and_special_tokens(tok, table):
    assert table.stop_ids == (tok.eos_id,)
    for special in (tok.bos_id, tok.eos_id, 2):
        assert table.pieces[special] == b""
    b = G.bind({"type": "json_object"}, tok, VOCAB)
    assert G.bind({"type": "json_object"}, tok, VOCAB) is b
    start, done = JSON.start_state, JSON.walk(JSON.start_state, b"{}")
    assert not b.token_allowed(start, tok.eos_id) and b.token_allowed(done, tok.eos_id)
    assert b.token_allowed(G.FIN, tok.eos_id) and b.token_allowed(G.DEAD, tok.eos_id)
    for st in (start, done, G.FIN, G.DEAD):
        assert not b.token_allowed(st, tok.bos_id) and not b.token_allowed(st, 2)          # never: zero bytes
        assert not b.token_allowed(st, VOCAB) and not b.token_allowed(st, -1)
    brace = table.pieces.index(b"{")
    assert b.token_allowed(start, brace) and not b.token_allowed(done, brace) and not b.token_allowed(G.FIN, brace)
    assert b.advance(start, tok.eos_id) == G.FIN and b.advance(G.FIN, brace) == G.FIN
    assert b.advance(done, brace) == G.DEAD and b.advance(G.DEAD, tok.eos_id) == G.DEAD
    assert b.advance(start, tok.bos_id) == G.DEAD
    assert b.state_after(tok.encode('{"a": [1, {"b": "c"}]}')) == done
    assert b.state_after(tok.encode('{"a": [1, {"b": "c"}]}') + [tok.eos_id, brace]) == G.FIN


def test_long_tokens_are_never_allowed():
    cap = G.GRAMMAR_TOKEN_BYTE_CAP
    pieces = [b"", b"a" * cap, b"a" * (cap + 1)] + [bytes([b]) for b in range(256)]
    t = G.TokenTable(pieces, [0])
    b = G.BoundGrammar(G.compile_grammar({"type": "regex", "pattern": "a*"}), t)
    st = b.g.start_state
    assert b.token_allowed(st, 1) and not b.token_allowed(st, 2) and b.token_allowed(st, 0)
    assert b.advance(st, 1)[0] >= 0 and b.advance(st, 2) == G.DEAD


def test_binding_refuses_a_vocabulary_without_the_quote_byte():
    pieces = [b""] + [bytes([b]) for b in range(256) if b != 0x22] + [b"ab", b"{}"]
    t = G.TokenTable(pieces, [0], name="no-quote")
    with pytest.raises(ValueError, match="cannot be bound"):
        G.BoundGrammar(JSON, t)
    G.BoundGrammar(G.compile_grammar({"type": "regex", "pattern": "[a-z]+"}), t)
    with pytest.raises(ValueError, match="stop id"):
        G.TokenTable(pieces, [])
    with pytest.raises(ValueError, match="neither byte-level nor Metaspace"):
        from tokenizers import Tokenizer, models
        wp = type("T", (), {"_tok": Tokenizer(models.WordLevel({"a": 0, "b": 1}, unk_token="a")), "stop_ids": {1},
                            "name": "wordlevel"})()
        G.token_table(wp, 2)


def test_metaspace_byte_fallback_vocabulary():
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers
    vocab = {"<unk>": 0, "</s>": 1}
    for b in range(256):
        vocab[f"<0x{b:02X}>"] = len(vocab)
    for w in ("▁", "▁yes", "no", '{"', "▁▁"):
        vocab[w] = len(vocab)
    t = Tokenizer(models.BPE(vocab, [], unk_token="<unk>", byte_fallback=True))
    t.pre_tokenizer = pre_tokenizers.Metaspace()
    t.decoder = decoders.Sequence([decoders.ByteFallback(), decoders.Metaspace()])
    t.add_special_tokens(["<unk>", "</s>"])
    hf = type("T", (), {"_tok": t, "stop_ids": frozenset({1}), "name": "sp"})()
    table = G.token_table(hf, len(vocab) + 3)
    assert table.pieces[0] == table.pieces[1] == b"" and table.pieces[-1] == b""       # specials, ids past the tokenizer
    assert table.pieces[2 + 0x22] == b'"' and table.pieces[2 + 0xE2] == b"\xe2"
    assert table.pieces[vocab["▁yes"]] == b" yes" and table.pieces[vocab["▁▁"]] == b"  "
    G.BoundGrammar(JSON, table)


# ---- the reference mask against the scalar walker ----------------------------------------------------------

PREFIXES = [b"", b"{", b'{"a', b'{"a\\', b'{"a\\u0', b'{"a\xe2', b'{"a\xf0\x9f', b'{"a"', b'{"a":', b'{"a":-', b'{"a":1',
            b'{"a":[1', b'{"a":[1.5e', b'{"a":tr', b'{"a":{"b":[[', b'{"a":1 ', b'{"a":[]', b'{}', b'{"a":' * CAP,
            b'{"a":' * (CAP - 1) + b"["]


def test_reference_mask_is_the_scalar_walk(tok, table):
    bound = G.bind({"type": "json_object"}, tok, VOCAB)
    rx = G.bind({"type": "regex", "pattern": r"-?\d+(\.\d+)?"}, tok, VOCAB)
    gm = ops.GrammarMask(3, "cpu", table)
    rng = random.Random(2)
    sample_ids = sorted(set(rng.sample(range(VOCAB), 3000)) | set(table.by_len[:300]) | {tok.eos_id, tok.bos_id})
    states = [JSON.walk(JSON.start_state, p) for p in PREFIXES] + [G.FIN, G.DEAD]
    assert all(s[0] >= 0 for s in states[:-2])
    for st in states:
        gm.fill([(bound, st), None, (rx, rx.g.start_state)])
        logits = torch.randn(3, VOCAB + 5)[:, :VOCAB]                             # row stride > V
        keep = logits.clone()
        ops.apply_grammar_mask(logits, gm)
        finite = ~torch.isinf(logits)
        assert torch.equal(logits[finite], keep[finite]) and torch.equal(logits[1], keep[1])
        assert bool((logits[~finite] == float("-inf")).all())
        assert finite[0].any() and finite[2].any()
        for i in sample_ids:
            assert bool(finite[0, i]) == bound.token_allowed(st, i), (st, i, table.pieces[i])
        assert int(finite[2].sum()) == sum(rx.token_allowed(rx.g.start_state, i) for i in range(VOCAB))
        row = ref.GrammarRow(gm, 0)
        for i in sample_ids[::40]:
            assert ref.grammar_advance(row, st, i, VOCAB) == bound.advance(st, i)
    assert gm.states(0)[0] == G.DEAD and gm.states(0)[2] == rx.g.start_state


def test_reference_graph_form_advances_the_two_slot_state(tok, table):
    bound = G.bind({"type": "json_object"}, tok, VOCAB)
    gm = ops.GrammarMask(2, "cpu", table).fill([(bound, JSON.start_state), None])
    ids = tok.encode('{"k": [true]}') + [tok.eos_id, tok.eos_id]
    out = torch.zeros(len(ids) + 1, 2, dtype=torch.int64)
    step = torch.zeros(1, dtype=torch.int64)
    st = JSON.start_state
    for s, t in enumerate(ids):
        logits = torch.zeros(2, VOCAB)
        ops.apply_grammar_mask(logits, gm, out, step)
        assert gm.states(s & 1)[0] == st or s == 0
        assert torch.isfinite(logits[0, t]) and bool(torch.isfinite(logits[1]).all())
        assert bool(torch.isfinite(logits[0, tok.eos_id])) == (bound.g.is_accepting(st) or st[0] < 0)
        out[s, 0] = t
        step += 1
        st = bound.advance(st, t)
    assert st == G.FIN


# ---- engine, serve ------------------------------------------------------------------------------------------

FINITE = {"type": "object", "properties": {
    "verdict": {"enum": ["yes", "no", "abstain"]}, "sure": {"type": "boolean"}, "version": {"const": 3},
    "why": {"type": "string", "maxLength": 4}}}
PROMPT = "Geef je oordeel als JSON."


def cpu_engine(**kw):
    cfg = dict(model="tiny-llama", device="cpu", dtype="fp32", num_blocks=256, weights="random:2")
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


def no_padding(engine) -> dict:
    """logit_bias banning the vocabulary's whitespace-only tokens (module docstring)."""
    t = engine.token_table()
    ban = {i: -100.0 for i, p in enumerate(t.pieces) if p and not p.strip(b" \t\n\r")}
    assert 0 < len(ban) <= 300
    return ban


@pytest.fixture(scope="module")
def engine():
    return cpu_engine()


def constrained(engine, grammar, n=120, **kw):
    kw.setdefault("temperature", 1.0)
    return SamplingParams(top_p=1.0, max_new_tokens=n, stop_on_consensus=False, grammar=grammar,
                          logit_bias=no_padding(engine), **kw)


def test_engine_reply_parses_validates_and_stops(engine):
    spec = {"type": "json_schema", "schema": FINITE}
    eos = engine.tokenizer.eos_id
    runs = []
    for _ in range(2):      # the same keys: a key is part of a row's seed
        outs = engine.run_turns([Turn(f"K{seed}", PROMPT, constrained(engine, spec, seed=seed)) for seed in (1, 2, 3)])
        for seed in (1, 2, 3):
            engine.release(f"K{seed}")
        runs.append([o.ids for o in outs])
        for o in outs:
            assert o.error is None and len(o.ids) < 60, o.text
            v = json.loads(o.text)
            assert validate(FINITE, v) and len(v["why"]) <= 4
            assert o.ids[-1] == eos and eos not in o.ids[:-1]      # the stop id ends the ids, not the text
    assert runs[0] == runs[1]
    assert len({tuple(r) for r in runs[0]}) > 1           # the seeds differ; the grammar does not fix the reply


def test_engine_sampled_ids_are_allowed_and_end_in_a_stop_id(engine):
    """The raw ids of a chunked decode (what serve runs): each is allowed at its state, the stop id
    comes well inside max_tokens, and only stop ids follow it."""
    spec = {"type": "json_schema", "schema": FINITE}
    turn = Turn("raw", PROMPT, constrained(engine, spec, n=200, seed=9, temperature=1.5))
    bound = G.bind(spec, engine.tokenizer, int(engine.cfg.vocab))
    (sq, first, _), = engine.start_turns([turn])
    gen = [first]
    eos = engine.tokenizer.eos_id
    while eos not in gen and len(gen) < 200:
        gen += engine.continue_decode([sq], [turn], [gen[-1]], 8)[0]
    gen += engine.continue_decode([sq], [turn], [gen[-1]], 4)[0]
    st = bound.g.start_state
    for t in gen:
        assert bound.token_allowed(st, t), (st, t)
        st = bound.advance(st, t)
    k = gen.index(eos)
    assert k < 150 and set(gen[k:]) == {eos} and st == G.FIN
    assert validate(FINITE, json.loads(engine.tokenizer.decode(gen[:k])))
    # json_object is no finite language (a random model may never close a string): every id is allowed,
    # and what max_tokens leaves is a live prefix of a document
    spec = {"type": "json_object"}
    o = engine.run_turns([Turn("obj", PROMPT, constrained(engine, spec, n=40, seed=1))])[0]
    bound = G.bind(spec, engine.tokenizer, int(engine.cfg.vocab))
    st = bound.g.start_state
    for t in o.ids:
        assert bound.token_allowed(st, t)
        st = bound.advance(st, t)
    assert st[0] >= 0 or st == G.FIN
    assert JSON.live(o.text.encode("utf-8")) and (st != G.FIN or isinstance(json.loads(o.text), dict))


def test_engine_mixed_batch_and_a_request_without_a_grammar(engine):
    other = cpu_engine()
    plain = SamplingParams(temperature=0.8, top_p=0.9, seed=4, max_new_tokens=12, ignore_eos=True, stop_on_consensus=False)
    want = other.run_turns([Turn("P", PROMPT, plain)])[0].ids
    engine.release("P")
    mixed = engine.run_turns([Turn("P", PROMPT, plain),
                              Turn("G", PROMPT, constrained(engine, {"type": "regex", "pattern": "(ja|nee)( (ja|nee)){2}"},
                                                            seed=5))])
    assert mixed[0].ids == want and len(want) == 12
    assert re.fullmatch("(ja|nee)( (ja|nee)){2}", mixed[1].text)
    engine.release("P")
    assert engine.run_turns([Turn("P", PROMPT, plain)])[0].ids == want


def test_engine_logprobs_report_the_mask(engine):
    spec = {"type": "json_schema", "schema": {"enum": ["yes", "no"]}}
    o = engine.run_turns([Turn("L", PROMPT, constrained(engine, spec, seed=2, logprobs=20))])[0]
    assert json.loads(o.text) in ("yes", "no")
    bound = G.bind(spec, engine.tokenizer, int(engine.cfg.vocab))
    st = bound.g.start_state
    for t, (lp, top_ids, top_lps) in zip(o.ids, o.logprobs):
        assert lp > float("-inf")
        for i, l in zip(top_ids, top_lps):
            assert (l == float("-inf")) == (not bound.token_allowed(st, i))
        st = bound.advance(st, t)


def test_engine_refuses_a_bad_grammar_before_prefill(engine, monkeypatch):
    """A spec the compiler refuses, ``ignore_eos`` with a grammar and a tokenizer that cannot be bound raise
    ValueError from the engine itself, before any prefill; the eager path keeps one mask per batch size."""
    def no_prefill(*a, **k):
        raise AssertionError("prefill ran")
    monkeypatch.setattr(engine, "_prefill_turns", no_prefill)
    bad = [SamplingParams(grammar={"type": "json_schema", "schema": {"type": "string", "pattern": "a"}}),
           SamplingParams(grammar={"type": "json_object"}, ignore_eos=True), SamplingParams(grammar={"type": "yaml"})]
    for p in bad:
        with pytest.raises(ValueError):
            engine._run_turns_ordered([Turn("bad", PROMPT, p)])
        with pytest.raises(ValueError):
            engine.start_turns([Turn("bad", PROMPT, p)])
    monkeypatch.setattr(G, "bind", lambda *a, **k: (_ for _ in ()).throw(ValueError("cannot be bound")))
    with pytest.raises(ValueError, match="cannot be bound"):
        engine.start_turns([Turn("bad", PROMPT, SamplingParams(grammar={"type": "json_object"}))])
    assert engine._grammar_mask(2, "cpu") is engine._grammar_mask(2, "cpu")
    assert engine._grammar_mask(3, "cpu") is not engine._grammar_mask(2, "cpu")


def test_bound_grammars_are_a_bounded_cache(tok, table, monkeypatch):
    monkeypatch.setattr(G, "_BOUND_CACHE", 3)
    first = G.bind({"type": "regex", "pattern": "a0"}, tok, VOCAB)
    assert G.bind({"type": "regex", "pattern": "a0"}, tok, VOCAB) is first
    for i in range(1, 5):
        G.bind({"type": "regex", "pattern": f"a{i}"}, tok, VOCAB)
    assert len(table._bound) == 3 and first.g.key not in table._bound
    assert G.bind({"type": "regex", "pattern": "a0"}, tok, VOCAB) is not first


def test_reply_text_drops_trailing_stop_ids_only(tok):
    from theroundtaible_amd.engine.engine import reply_text
    ids = tok.encode('{"a": 1}')
    with_grammar, plain = SamplingParams(grammar={"type": "json_object"}), SamplingParams()
    assert reply_text(tok, ids + [tok.eos_id, tok.eos_id], with_grammar) == '{"a": 1}'
    assert reply_text(tok, [tok.eos_id] + ids + [tok.eos_id], with_grammar) == tok.decode([tok.eos_id] + ids)
    assert reply_text(tok, ids + [tok.eos_id], plain) == tok.decode(ids + [tok.eos_id])


def test_dist_greedy_is_off_for_a_batch_with_a_grammar():
    from theroundtaible_amd.parallel.tp import TPInfo
    e = object.__new__(Engine)
    e.tp = TPInfo(size=2, rank=0)
    e.on_gpu = False
    e.ecfg = EngineConfig(device="cpu")
    greedy = lambda **kw: SamplingParams(temperature=0.0, **kw)      # noqa: E731
    plain, gr = Turn("a", "x", greedy()), Turn("b", "x", greedy(grammar={"type": "json_object"}))
    assert e.dist_greedy([plain, plain]) is True and e.dist_greedy([plain, gr]) is False
    key = (8, 4, False, False)
    assert Engine._cache_key(key, False, False) == key and Engine._cache_key(key, False, False, False) == key
    assert Engine._cache_key(key, True, True, True) == (key, "proc", "gr", "lp")
    assert Engine._cache_key(key, False, False, True) == (key, "gr")


@pytest.fixture(scope="module")
def server():
    srv = build_server("tiny-llama", weights="random:1", device="cpu", port=0, max_batch=4, max_tokens=96,
                       num_blocks=512).start()
    yield srv
    srv.close()


def closing(engine, ban: dict) -> dict:
    """``ban`` plus a strong bias towards the tokens ``}`` and ``{}``: json_object is no finite language, and
    a random model closes the object only when pushed to."""
    t = engine.token_table()
    return {**ban, t.pieces.index(b"}"): 100.0, t.pieces.index(b"{}"): 100.0}


def _post(url, body):
    req = urllib.request.Request(url, data=json.dumps(body).encode(), method="POST",
                                 headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(req, timeout=300) as r:
        return r.status, r.read().decode()


def _stream_text(url, body):
    req = urllib.request.Request(url + "/v1/completions", data=json.dumps(dict(body, stream=True)).encode(), method="POST",
                                 headers={"Content-Type": "application/json"})
    text, finish = "", None
    with urllib.request.urlopen(req, timeout=300) as r:
        for raw in r:
            line = raw.decode().strip()
            if line.startswith("data: ") and line != "data: [DONE]":
                c = json.loads(line[6:])["choices"][0]
                text += c["text"]
                finish = c["finish_reason"] or finish
    return text, finish


def test_serve_response_format_and_guided_regex(server):
    ban = {str(k): v for k, v in no_padding(server.engine).items()}
    base = {"max_tokens": 96, "temperature": 1.0, "seed": 7, "logit_bias": ban}
    code, reply = _post(server.url + "/v1/completions", dict(base, prompt=PROMPT, response_format={
        "type": "json_schema", "json_schema": {"name": "verdict", "schema": FINITE}}))
    choice = json.loads(reply)["choices"][0]
    assert code == 200 and choice["finish_reason"] == "stop" and validate(FINITE, json.loads(choice["text"]))
    base_obj = dict(base, logit_bias={str(k): v for k, v in closing(server.engine, no_padding(server.engine)).items()})
    body = dict(base_obj, prompt=PROMPT, response_format={"type": "json_object"})
    code, reply = _post(server.url + "/v1/completions", body)
    choice = json.loads(reply)["choices"][0]
    assert code == 200 and choice["finish_reason"] == "stop" and isinstance(json.loads(choice["text"]), dict)
    assert _stream_text(server.url, body) == (choice["text"], "stop")       # streamed pieces concatenate to the same text
    msgs = [{"role": "user", "content": PROMPT}]
    code, reply = _post(server.url + "/v1/chat/completions", dict(base_obj, messages=msgs, response_format={"type": "json_object"}))
    assert code == 200 and isinstance(json.loads(json.loads(reply)["choices"][0]["message"]["content"]), dict)
    pattern = r"(ja|nee), want [a-z]{1,5}\."
    code, reply = _post(server.url + "/v1/chat/completions", dict(base, messages=msgs, guided_regex=pattern, logprobs=True,
                                                                  top_logprobs=3))
    choice = json.loads(reply)["choices"][0]
    assert code == 200 and re.fullmatch(pattern, choice["message"]["content"])
    assert all(e["logprob"] > -9999.0 for e in choice["logprobs"]["content"])
    # {"type": "text"} and an absent field: no grammar, the same ids
    plain = {"prompt": PROMPT, "max_tokens": 8, "temperature": 0, "ignore_eos": True}
    assert server.sampling(plain).grammar is None and server.sampling(dict(plain, response_format={"type": "text"})).grammar is None
    a, _ = server.generate(PROMPT, plain, None)
    b, _ = server.generate(PROMPT, dict(plain, response_format={"type": "text"}), None)
    assert a.ids == b.ids and len(a.ids) == 8
    # max_tokens cuts a document short: finish_reason "length"
    code, reply = _post(server.url + "/v1/completions", dict(base, prompt=PROMPT, max_tokens=2, response_format={
        "type": "json_schema", "json_schema": {"schema": FINITE}}))
    choice = json.loads(reply)["choices"][0]
    assert choice["finish_reason"] == "length" and G.compile_grammar({"type": "json_schema", "schema": FINITE}).live(
        choice["text"].encode())


def test_serve_ollama_format(server):
    ban = closing(server.engine, no_padding(server.engine))
    real = server.sampling
    msgs = [{"role": "user", "content": PROMPT}]
    opts = {"num_predict": 96, "temperature": 1.0, "seed": 3}
    try:     # Ollama's options carry no logit_bias: the padding ban is added where the request becomes params
        server.sampling = lambda body: SamplingParams(**{**real(body).__dict__, "logit_bias": ban})
        code, reply = _post(server.url + "/api/chat", {"messages": msgs, "stream": False, "format": "json", "options": opts})
        assert code == 200 and isinstance(json.loads(json.loads(reply)["message"]["content"]), dict)
        code, reply = _post(server.url + "/api/chat", {"messages": msgs, "stream": False, "format": FINITE, "options": opts})
        assert code == 200 and validate(FINITE, json.loads(json.loads(reply)["message"]["content"]))
    finally:
        server.sampling = real
    assert server.sampling({"format": "json"}).grammar == {"type": "json_object"}
    assert server.sampling({"format": FINITE}).grammar == {"type": "json_schema", "schema": FINITE}


BAD = [
    ("unsupported keyword", {"response_format": {"type": "json_schema", "json_schema": {"schema": {"type": "string", "pattern": "a"}}}},
     "pattern"),
    ("$ref", {"response_format": {"type": "json_schema", "json_schema": {"schema": {"$ref": "#"}}}}, "$ref"),
    ("over the state cap", {"guided_regex": "[a-z]{900}[0-9]{900}[a-z]{900}[0-9]{900}[a-z]{900}"}, "states"),
    ("bad regex", {"guided_regex": "(a"}, "regex"),
    ("regex not a string", {"guided_regex": ["a"]}, "guided_regex"),
    ("two fields", {"guided_regex": "a+", "response_format": {"type": "json_object"}}, "only one of"),
    ("unknown response_format", {"response_format": {"type": "yaml"}}, "response_format"),
    ("schema missing", {"response_format": {"type": "json_schema"}}, "json_schema"),
    ("ignore_eos", {"response_format": {"type": "json_object"}, "ignore_eos": True}, "ignore_eos"),
]


@pytest.mark.parametrize("name,extra,message", BAD, ids=[b[0] for b in BAD])
def test_serve_bad_grammar_requests_get_400(server, name, extra, message):
    for path, body in (("/v1/completions", {"prompt": "x", "max_tokens": 2}),
                       ("/v1/chat/completions", {"messages": [{"role": "user", "content": "x"}], "max_tokens": 2,
                                                 "stream": True})):
        with pytest.raises(urllib.error.HTTPError) as ei:
            _post(server.url + path, dict(body, **extra))
        assert ei.value.code == 400
        err = json.loads(ei.value.read().decode())["error"]
        assert err["type"] == "invalid_request_error" and message in err["message"]


def test_serve_ollama_bad_format_and_unbindable_tokenizer_get_400(server, monkeypatch):
    msgs = [{"role": "user", "content": "q"}]
    for fmt in ("yaml", 3, {"type": "string", "format": "date"}):
        with pytest.raises(urllib.error.HTTPError) as ei:
            _post(server.url + "/api/chat", {"messages": msgs, "stream": False, "format": fmt})
        assert ei.value.code == 400

    def refuse(*a, **k):
        raise ValueError("the json_object grammar cannot be bound to tokenizer 'x'")
    monkeypatch.setattr(G, "bind", refuse)
    with pytest.raises(urllib.error.HTTPError) as ei:
        _post(server.url + "/v1/completions", {"prompt": "x", "max_tokens": 2, "response_format": {"type": "json_object"}})
    assert ei.value.code == 400 and "cannot be bound" in json.loads(ei.value.read().decode())["error"]["message"]
