"""Grammar-constrained decoding: byte-level automata for JSON, a JSON-schema subset and a regex subset.

Every grammar compiles to ONE form (:class:`CompiledGrammar`), the form the mask kernel
(csrc/grammar_mask.hip, walk: csrc/grammar_core.h) reads:

* a 256-entry byte -> class map and ``trans[n_states * n_classes]`` of 16-bit entries: ``0xFFFF`` is
  dead, anything else ``(q' << 2) | action`` with action none / push 0 / push 1 / pop;
* a state of the walk is ``(q, depth, stack)``: ``stack`` holds one bit per open container
  (0 = object, 1 = array; bit ``depth - 1`` is the top) in a 32-bit word. A push at
  ``GRAMMAR_MAX_DEPTH`` is dead; a pop on an empty stack is dead; a pop removes the top bit and goes
  to ``pop_target[0 | 1 | 2]`` for an object / an array / nothing then on top — the only transition
  that reads the stack. Everything else about the context is folded into ``q``;
* ``accept[q]``; ``Q_FIN`` (a stop id was consumed) and ``Q_DEAD`` (a walk died) allow stop ids only.

Regular grammars (regex, schema) use no actions. The automata work on BYTES: a token that splits a
UTF-8 code point needs no special case, the string states track the sequence.

Front ends: ``{"type": "json_object"}``, ``{"type": "regex", "pattern": ...}``,
``{"type": "json_schema", "schema": ...}`` and ``{"type": "tail", "open": ..., "body": <schema or regex
spec>, "close": ...}``: free bytes up to the first ``open``, then the body, then ``close`` (see
:func:`compile_grammar`). Whitespace between JSON
tokens is unbounded in all of them: a model may pad, and ``max_new_tokens`` bounds it.

Regex subset (anchored at both ends): literals and escapes (``\\n \\t \\r \\f \\v \\0 \\xHH \\uHHHH``
and escaped punctuation), ``.`` (any code point but ``\\n``), classes and negated classes with ranges,
``\\d \\w \\s`` and ``\\D \\W \\S`` (ASCII definitions), groups ``( )`` / ``(?: )``, ``|``,
``* + ? {m} {m,} {m,n}``. Non-ASCII literals match their UTF-8 bytes; ``.`` and negated classes match
whole well-formed UTF-8 code points. Not supported (ValueError): anchors, back-references,
look-around, lazy / possessive quantifiers, flags.

Schema subset: see :func:`schema_to_ast`.
"""
from __future__ import annotations

import functools
import json
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

GRAMMAR_MAX_DEPTH = 32            # open containers; the stack is one 32-bit word
GRAMMAR_MAX_STATES = 4096         # q' takes 12 of an entry's 16 bits beside the 2 action bits
GRAMMAR_MAX_CLASSES = 64
GRAMMAR_MAX_TABLE = 65536         # n_states * n_classes entries (128 KiB per batch row on the device)
GRAMMAR_TOKEN_BYTE_CAP = 128      # a longer token is never allowed under a grammar
GRAMMAR_MAX_STOPS = 8             # stop ids a row can name
Q_FIN, Q_DEAD = -1, -2
DEAD_ENTRY = 0xFFFF
ACT_NONE, ACT_PUSH0, ACT_PUSH1, ACT_POP = 0, 1, 2, 3
_DFA_BLOWUP = 8 * GRAMMAR_MAX_STATES     # subset construction gives up here (before minimisation)
_BOUND_CACHE = 256                       # bound grammars kept per token table, like compiled ones
TAIL_MAX_BYTES = 32               # a tail grammar's opener and closer
NEED_INF16 = 0xFFFF               # a 16-bit need entry: no path through single-byte tokens
NEED_INF = 1 << 30                # need() of a state with such an entry on its way
BUDGET_FREE = 1 << 29             # a row's budget when nothing bounds it (grammar_finish off)

State = Tuple[int, int, int]      # (q, depth, stack)
DEAD: State = (Q_DEAD, 0, 0)
FIN: State = (Q_FIN, 0, 0)


class CompiledGrammar:
    """The compiled form (module docstring). ``trans`` is flat, row-major ``[n_states][n_classes]``."""

    def __init__(self, kind: str, key: str, cls: bytes, n_classes: int, trans: List[int], accept: bytes,
                 pop_target: Tuple[int, int, int], start: int):
        self.kind, self.key = kind, key
        self.cls, self.n_classes, self.trans, self.accept = cls, n_classes, trans, accept
        self.n_states = len(accept)
        self.pop_target, self.start = pop_target, start
        self.uses_stack = any(e != DEAD_ENTRY and (e & 3) for e in trans)

    @property
    def start_state(self) -> State:
        return (self.start, 0, 0)

    def walk(self, state: State, data: bytes) -> State:
        """Advance ``state`` over ``data``; ``DEAD`` when a byte has no transition. ``FIN`` / ``DEAD`` stay."""
        q, depth, stack = state
        if q < 0:
            return state
        ncls, trans, cls, pops = self.n_classes, self.trans, self.cls, self.pop_target
        for byte in data:
            e = trans[q * ncls + cls[byte]]
            if e == DEAD_ENTRY:
                return DEAD
            act = e & 3
            if act == ACT_POP:
                if depth == 0:
                    return DEAD
                depth -= 1
                stack &= ~(1 << depth)
                q = pops[2 if depth == 0 else (stack >> (depth - 1)) & 1]
                if q < 0:
                    return DEAD
            else:
                if act:
                    if depth == GRAMMAR_MAX_DEPTH:
                        return DEAD
                    stack |= (act - 1) << depth
                    depth += 1
                q = e >> 2
        return (q, depth, stack)

    def is_accepting(self, state: State) -> bool:
        return state[0] >= 0 and bool(self.accept[state[0]])

    def accepts(self, data: bytes) -> bool:
        return self.is_accepting(self.walk(self.start_state, data))

    def live(self, data: bytes) -> bool:
        return self.walk(self.start_state, data)[0] >= 0

    def reaches_accept(self) -> List[bool]:
        """Per state: some path (a pop may go to any pop target) ends in an accepting state."""
        rev: List[set] = [set() for _ in range(self.n_states)]
        for q in range(self.n_states):
            for c in range(self.n_classes):
                e = self.trans[q * self.n_classes + c]
                if e == DEAD_ENTRY:
                    continue
                for t in ([p for p in self.pop_target if p >= 0] if (e & 3) == ACT_POP else [e >> 2]):
                    rev[t].add(q)
        good = [bool(a) for a in self.accept]
        todo = [q for q, a in enumerate(good) if a]
        while todo:
            for p in rev[todo.pop()]:
                if not good[p]:
                    good[p] = True
                    todo.append(p)
        return good


# ---- from per-state byte edges to the compiled form -----------------------------------------------------

def _finish(kind: str, key: str, rows: List[Dict[int, Tuple[int, int]]], accept: Sequence[bool], start: int,
            pop_target: Tuple[int, int, int] = (-1, -1, -1)) -> CompiledGrammar:
    """``rows[q][byte] = (q', action)``. Trims (keeps states reachable from ``start`` that reach accept),
    merges bytes with equal columns into classes, checks the caps and encodes."""
    n = len(rows)
    pops = [p for p in pop_target if p >= 0]

    def succ(q: int) -> set:
        out = set()
        for t, a in rows[q].values():
            out.update(pops) if a == ACT_POP else out.add(t)
        return out

    fwd, todo = {start}, [start]
    while todo:
        for t in succ(todo.pop()):
            if t not in fwd:
                fwd.add(t)
                todo.append(t)
    rev: List[set] = [set() for _ in range(n)]
    for q in fwd:
        for t in succ(q):
            rev[t].add(q)
    good = {q for q in fwd if accept[q]}
    todo = list(good)
    while todo:
        for p in rev[todo.pop()]:
            if p not in good:
                good.add(p)
                todo.append(p)
    if start not in good:
        raise ValueError("the grammar accepts nothing")
    order = sorted(good)
    new = {q: i for i, q in enumerate(order)}
    if len(order) > GRAMMAR_MAX_STATES:
        raise ValueError(f"the grammar needs {len(order)} states; at most {GRAMMAR_MAX_STATES} are supported")
    cols: Dict[tuple, int] = {}
    cls = bytearray(256)
    table: List[List[int]] = []          # per class, the column
    for byte in range(256):
        col = []
        for q in order:
            e = rows[q].get(byte)
            if e is None or (e[1] != ACT_POP and e[0] not in new):
                col.append(DEAD_ENTRY)
            else:
                col.append(ACT_POP if e[1] == ACT_POP else (new[e[0]] << 2) | e[1])
        sig = tuple(col)
        if sig not in cols:
            cols[sig] = len(table)
            table.append(col)
        cls[byte] = cols[sig]
    ncls = len(table)
    if ncls > GRAMMAR_MAX_CLASSES:
        raise ValueError(f"the grammar needs {ncls} byte classes; at most {GRAMMAR_MAX_CLASSES} are supported")
    if ncls * len(order) > GRAMMAR_MAX_TABLE:
        raise ValueError(f"the grammar's table has {ncls * len(order)} entries; at most {GRAMMAR_MAX_TABLE} "
                         f"are supported")
    trans = [table[c][i] for i in range(len(order)) for c in range(ncls)]
    return CompiledGrammar(kind, key, bytes(cls), ncls, trans, bytes(1 if accept[q] else 0 for q in order),
                           tuple(new.get(p, -1) for p in pop_target), new[start])


# ---- json_object ----------------------------------------------------------------------------------------

_WS = b" \t\n\r"                 # RFC 8259 whitespace
_DIGITS = b"0123456789"
_HEX = b"0123456789abcdefABCDEF"


def _build_json(key: str) -> CompiledGrammar:
    names: Dict[str, int] = {}
    rows: List[Dict[int, Tuple[int, int]]] = []

    def s(name: str) -> int:
        if name not in names:
            names[name] = len(rows)
            rows.append({})
        return names[name]

    def add(src: str, data: Iterable[int], dst: Optional[str], act: int = ACT_NONE) -> None:
        r = rows[s(src)]
        t = s(dst) if dst is not None else 0
        for byte in data:
            assert byte not in r, (src, byte)
            r[byte] = (t, act)

    cont = range(0x80, 0xC0)
    add("start", _WS, "start")
    add("start", b"{", "obj_open", ACT_PUSH0)
    add("obj_open", _WS, "obj_open")
    add("obj_open", b'"', "str_key")
    add("obj_open", b"}", None, ACT_POP)
    add("obj_key", _WS, "obj_key")
    add("obj_key", b'"', "str_key")
    add("after_key", _WS, "after_key")
    add("after_key", b":", "val_obj")
    # strings: the context (key / value in an object / value in an array) picks the state after the quote.
    # UTF-8 is well formed: no overlong forms, no surrogates, nothing past U+10FFFF.
    for c, after in (("key", "after_key"), ("obj", "after_obj"), ("arr", "after_arr")):
        S = "str_" + c
        add(S, [b for b in range(0x20, 0x80) if b not in (0x22, 0x5C)], S)
        add(S, b'"', after)
        add(S, b"\\", "esc_" + c)
        add("esc_" + c, b'"\\/bfnrt', S)
        add("esc_" + c, b"u", "u1_" + c)
        for i in range(1, 5):
            add(f"u{i}_{c}", _HEX, f"u{i + 1}_{c}" if i < 4 else S)
        add(S, range(0xC2, 0xE0), "c1_" + c)
        add(S, [0xE0], "e0_" + c)
        add(S, [*range(0xE1, 0xED), 0xEE, 0xEF], "c2_" + c)
        add(S, [0xED], "ed_" + c)
        add(S, [0xF0], "f0_" + c)
        add(S, range(0xF1, 0xF4), "c3_" + c)
        add(S, [0xF4], "f4_" + c)
        add("c1_" + c, cont, S)
        add("c2_" + c, cont, "c1_" + c)
        add("e0_" + c, range(0xA0, 0xC0), "c1_" + c)
        add("ed_" + c, range(0x80, 0xA0), "c1_" + c)
        add("c3_" + c, cont, "c2_" + c)
        add("f0_" + c, range(0x90, 0xC0), "c2_" + c)
        add("f4_" + c, range(0x80, 0x90), "c2_" + c)
    for c, closer, nxt in (("obj", b"}", "obj_key"), ("arr", b"]", "val_arr")):
        after = "after_" + c

        def value(src: str) -> None:
            add(src, _WS, src)
            add(src, b'"', "str_" + c)
            add(src, b"{", "obj_open", ACT_PUSH0)
            add(src, b"[", "arr_open", ACT_PUSH1)
            add(src, b"-", "minus_" + c)
            add(src, b"0", "zero_" + c)
            add(src, b"123456789", "int_" + c)
            add(src, b"t", "t1_" + c)
            add(src, b"f", "f1_" + c)
            add(src, b"n", "n1_" + c)

        value("val_" + c)
        if c == "arr":
            value("arr_open")
            add("arr_open", b"]", None, ACT_POP)
        add(after, _WS, after)
        add(after, b",", nxt)
        add(after, closer, None, ACT_POP)
        add("minus_" + c, b"0", "zero_" + c)
        add("minus_" + c, b"123456789", "int_" + c)
        add("int_" + c, _DIGITS, "int_" + c)
        for st in ("zero_", "int_"):
            add(st + c, b".", "frac0_" + c)
            add(st + c, b"eE", "exp0_" + c)
        add("frac0_" + c, _DIGITS, "frac_" + c)
        add("frac_" + c, _DIGITS, "frac_" + c)
        add("frac_" + c, b"eE", "exp0_" + c)
        add("exp0_" + c, b"+-", "expsign_" + c)
        add("exp0_" + c, _DIGITS, "exp_" + c)
        add("expsign_" + c, _DIGITS, "exp_" + c)
        add("exp_" + c, _DIGITS, "exp_" + c)
        for st in ("zero_", "int_", "frac_", "exp_"):     # a number ends at whatever may follow a value
            add(st + c, _WS, after)
            add(st + c, b",", nxt)
            add(st + c, closer, None, ACT_POP)
        for word in (b"true", b"false", b"null"):
            p = chr(word[0])
            for i in range(1, len(word)):
                add(f"{p}{i}_{c}", word[i:i + 1], f"{p}{i + 1}_{c}" if i + 1 < len(word) else after)
    s("done")        # after the closing brace at depth 0: only a stop id
    accept = [False] * len(rows)
    accept[names["done"]] = True
    g = _finish("json_object", key, rows, accept, names["start"],
                (names["after_obj"], names["after_arr"], names["done"]))
    g.names = {n: q for n, q in names.items()}      # trimming keeps every state here, in order
    assert g.n_states == len(rows)
    return g


# ---- regex: parser -> AST -> NFA -> DFA -> trim -> minimise ---------------------------------------------
# AST: ("set", 256-bit int mask) one byte | ("cat", [..]) | ("alt", [..]) | ("rep", node, m, n or None)

_MAX_CP = 0x10FFFF
_ASCII_D = [(0x30, 0x39)]
_ASCII_W = [(0x30, 0x39), (0x41, 0x5A), (0x5F, 0x5F), (0x61, 0x7A)]
_ASCII_S = [(0x09, 0x0D), (0x20, 0x20)]
_REP_MAX = 1000


def _mask(data: Iterable[int]) -> int:
    m = 0
    for b in data:
        m |= 1 << b
    return m


def lit(data: bytes):
    return ("cat", [("set", 1 << b) for b in data])


def _norm_ranges(ranges):
    out: List[List[int]] = []
    for lo, hi in sorted(ranges):
        if out and lo <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [(a, b) for a, b in out]


def _negate(ranges):
    out, prev = [], 0
    for lo, hi in _norm_ranges(ranges):
        if lo > prev:
            out.append((prev, lo - 1))
        prev = hi + 1
    if prev <= _MAX_CP:
        out.append((prev, _MAX_CP))
    return out


def _utf8_split(lo: int, hi: int):
    """Sequences of byte ranges matching exactly the code points lo..hi (one encoded length)."""
    if hi <= 0x7F:
        yield [(lo, hi)]
        return
    for i in (1, 2, 3):
        m = (1 << (6 * i)) - 1
        if (lo & ~m) != (hi & ~m):
            if lo & m:
                yield from _utf8_split(lo, lo | m)
                yield from _utf8_split((lo | m) + 1, hi)
                return
            if (hi & m) != m:
                yield from _utf8_split(lo, (hi & ~m) - 1)
                yield from _utf8_split(hi & ~m, hi)
                return
    yield list(zip(chr(lo).encode("utf-8"), chr(hi).encode("utf-8")))


def cp_class(ranges):
    """AST matching one code point of ``ranges`` (surrogates excluded) as well-formed UTF-8."""
    alts = []
    for lo, hi in _norm_ranges(ranges):
        for a, b in ((0, 0x7F), (0x80, 0x7FF), (0x800, 0xD7FF), (0xE000, 0xFFFF), (0x10000, _MAX_CP)):
            l, h = max(lo, a), min(hi, b)
            if l <= h:
                for seq in _utf8_split(l, h):
                    alts.append(("cat", [("set", _mask(range(x, y + 1))) for x, y in seq]))
    if not alts:
        raise ValueError("empty character class")
    ascii_mask = 0
    rest = []
    for a in alts:      # one set for the single-byte part keeps the NFA small
        if len(a[1]) == 1:
            ascii_mask |= a[1][0][1]
        else:
            rest.append(a)
    if ascii_mask:
        rest.insert(0, ("set", ascii_mask))
    return rest[0] if len(rest) == 1 else ("alt", rest)


class _RegexParser:
    def __init__(self, pattern: str):
        self.p, self.i = pattern, 0

    def err(self, msg: str):
        return ValueError(f"regex: {msg} at position {self.i} of {self.p!r}")

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            raise self.err("unbalanced ')'")
        return node

    def alt(self):
        items = [self.cat()]
        while self.i < len(self.p) and self.p[self.i] == "|":
            self.i += 1
            items.append(self.cat())
        return items[0] if len(items) == 1 else ("alt", items)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.p[self.i] not in "|)":
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self):
        node = self.atom()
        while self.i < len(self.p) and self.p[self.i] in "*+?{":
            ch = self.p[self.i]
            if ch == "{":
                j = self.p.find("}", self.i)
                body = self.p[self.i + 1:j] if j > 0 else ""
                parts = body.split(",")
                if j < 0 or len(parts) > 2 or not parts[0].isdigit() or (len(parts) == 2 and parts[1]
                                                                          and not parts[1].isdigit()):
                    raise self.err("bad repetition")
                m = int(parts[0])
                n = m if len(parts) == 1 else (int(parts[1]) if parts[1] else None)
                if m > _REP_MAX or (n is not None and (n > _REP_MAX or n < m)):
                    raise self.err("bad repetition bounds")
                self.i = j + 1
            else:
                m, n = {"*": (0, None), "+": (1, None), "?": (0, 1)}[ch]
                self.i += 1
            if self.i < len(self.p) and self.p[self.i] in "?+":
                raise self.err("lazy and possessive quantifiers are not supported")
            node = ("rep", node, m, n)
        return node

    def escape(self):
        """After a backslash: ("ranges", [...], negated) or ("cp", code point)."""
        if self.i >= len(self.p):
            raise self.err("trailing backslash")
        ch = self.p[self.i]
        self.i += 1
        if ch in "dDwWsS":
            return ("ranges", {"d": _ASCII_D, "w": _ASCII_W, "s": _ASCII_S}[ch.lower()], ch.isupper())
        simple = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11, "0": 0, "a": 7}
        if ch in simple:
            return ("cp", simple[ch])
        if ch in "xu":
            n = 2 if ch == "x" else 4
            h = self.p[self.i:self.i + n]
            if len(h) != n or any(c not in "0123456789abcdefABCDEF" for c in h):
                raise self.err("bad hex escape")
            self.i += n
            return ("cp", int(h, 16))
        if ch.isalnum():
            raise self.err(f"unsupported escape \\{ch}")
        return ("cp", ord(ch))

    def atom(self):
        ch = self.p[self.i]
        if ch == "(":
            self.i += 1
            if self.p.startswith("?:", self.i):
                self.i += 2
            elif self.p.startswith("?", self.i):
                raise self.err("only (?: ) groups are supported")
            node = self.alt()
            if self.i >= len(self.p) or self.p[self.i] != ")":
                raise self.err("missing ')'")
            self.i += 1
            return node
        if ch == "[":
            return self.char_class()
        if ch == ".":
            self.i += 1
            return cp_class(_negate([(10, 10)]))
        if ch in "^$":
            raise self.err("anchors are not supported (the pattern is anchored at both ends)")
        if ch in "*+?{":
            raise self.err("nothing to repeat")
        if ch == "\\":
            self.i += 1
            e = self.escape()
            if e[0] == "cp":
                return lit(chr(e[1]).encode("utf-8"))
            return cp_class(_negate(e[1]) if e[2] else e[1])
        self.i += 1
        return lit(ch.encode("utf-8"))

    def char_class(self):
        self.i += 1
        neg = self.i < len(self.p) and self.p[self.i] == "^"
        self.i += neg
        ranges, first = [], True
        while True:
            if self.i >= len(self.p):
                raise self.err("missing ']'")
            ch = self.p[self.i]
            if ch == "]" and not first:
                self.i += 1
                break
            first = False
            self.i += 1
            if ch == "\\":
                e = self.escape()
                if e[0] == "ranges":
                    ranges += _negate(e[1]) if e[2] else e[1]
                    continue
                lo = e[1]
            else:
                lo = ord(ch)
            if self.i + 1 < len(self.p) and self.p[self.i] == "-" and self.p[self.i + 1] != "]":
                self.i += 1
                ch2 = self.p[self.i]
                self.i += 1
                if ch2 == "\\":
                    e = self.escape()
                    if e[0] != "cp":
                        raise self.err("bad range")
                    hi = e[1]
                else:
                    hi = ord(ch2)
                if hi < lo:
                    raise self.err("bad range")
                ranges.append((lo, hi))
            else:
                ranges.append((lo, lo))
        return cp_class(_negate(ranges) if neg else ranges)


def parse_regex(pattern: str):
    if not isinstance(pattern, str):
        raise ValueError("regex: the pattern must be a string")
    return _RegexParser(pattern).parse()


def _ast_to_grammar(kind: str, key: str, ast, opener: bytes = b"") -> CompiledGrammar:
    """``opener``: the language becomes any bytes up to and including the FIRST occurrence of ``opener``,
    then ``L(ast)`` (the ``tail`` grammar): the opener's KMP prefix automaton, total on all 256 bytes,
    stands in front of the NFA, and the subset construction takes tokens across the seam."""
    eps: List[List[int]] = []
    edges: List[List[Tuple[int, int]]] = []      # (byte mask, target)

    def new() -> int:
        eps.append([])
        edges.append([])
        if len(eps) > 64 * GRAMMAR_MAX_STATES:
            raise ValueError("the grammar is too large (NFA)")
        return len(eps) - 1

    def build(node) -> Tuple[int, int]:
        op = node[0]
        if op == "set":
            a, b = new(), new()
            edges[a].append((node[1], b))
            return a, b
        if op == "cat":
            a = b = new()
            for it in node[1]:
                x, y = build(it)
                eps[b].append(x)
                b = y
            return a, b
        if op == "alt":
            a, b = new(), new()
            for it in node[1]:
                x, y = build(it)
                eps[a].append(x)
                eps[y].append(b)
            return a, b
        _, sub, m, n = node
        a = b = new()
        for _ in range(m):
            x, y = build(sub)
            eps[b].append(x)
            b = y
        if n is None:
            x, y = build(sub)
            h = new()
            eps[b].append(h)
            eps[h].append(x)
            eps[y].append(h)
            b = h
        else:
            end = new()
            for _ in range(n - m):
                x, y = build(sub)
                eps[b].append(x)
                eps[b].append(end)
                b = y
            eps[b].append(end)
            b = end
        return a, b

    n_start, n_end = build(ast)
    if opener:
        m = len(opener)
        fail = [0] * (m + 1)          # fail[i]: the longest proper border of opener[:i]
        for i in range(1, m):
            k = fail[i]
            while k and opener[i] != opener[k]:
                k = fail[k]
            fail[i + 1] = k + 1 if opener[i] == opener[k] else 0
        free = [new() for _ in range(m)]
        for i in range(m):
            masks_to: Dict[int, int] = {}
            for byte in range(256):
                k = i
                while k and opener[k] != byte:
                    k = fail[k]
                k = k + 1 if opener[k] == byte else 0
                masks_to[k] = masks_to.get(k, 0) | (1 << byte)
            for k, mk in masks_to.items():
                edges[free[i]].append((mk, n_start if k == m else free[k]))
        n_start = free[0]
    # byte classes of the NFA's masks: subset construction runs per class, not per byte
    masks = sorted({m for es in edges for m, _ in es})
    sig: Dict[tuple, int] = {}
    bcls = []
    for byte in range(256):
        k = tuple(i for i, m in enumerate(masks) if (m >> byte) & 1)
        bcls.append(sig.setdefault(k, len(sig)))
    rep = {}
    for byte, c in enumerate(bcls):
        rep.setdefault(c, byte)
    mask_cls = {m: [c for c, byte in rep.items() if (m >> byte) & 1] for m in masks}

    def closure(states) -> frozenset:
        seen, todo = set(states), list(states)
        while todo:
            for t in eps[todo.pop()]:
                if t not in seen:
                    seen.add(t)
                    todo.append(t)
        return frozenset(seen)

    d0 = closure([n_start])
    ids = {d0: 0}
    drows: List[Dict[int, int]] = []
    order = [d0]
    k = 0
    while k < len(order):
        cur = order[k]
        k += 1
        move: Dict[int, set] = {}
        for st in cur:
            for m, t in edges[st]:
                for c in mask_cls[m]:
                    move.setdefault(c, set()).add(t)
        row = {}
        memo: Dict[frozenset, int] = {}
        for c, ts in move.items():
            fs = frozenset(ts)
            if fs not in memo:
                d = closure(fs)
                if d not in ids:
                    ids[d] = len(order)
                    order.append(d)
                    if len(order) > _DFA_BLOWUP:
                        raise ValueError(f"the grammar needs more than {_DFA_BLOWUP} states before minimisation; "
                                         f"at most {GRAMMAR_MAX_STATES} are supported")
                memo[fs] = ids[d]
            row[c] = memo[fs]
        drows.append(row)
    acc = [n_end in d for d in order]
    # trim: states that cannot reach accept go (their edges become dead)
    rev: List[set] = [set() for _ in order]
    for q, row in enumerate(drows):
        for t in row.values():
            rev[t].add(q)
    good = {q for q, a in enumerate(acc) if a}
    todo = list(good)
    while todo:
        for p in rev[todo.pop()]:
            if p not in good:
                good.add(p)
                todo.append(p)
    if 0 not in good:
        raise ValueError("the grammar accepts nothing")
    ncls = len(sig)
    # minimise (Moore): refine {accepting, not} by the blocks of the successors until stable
    # (seeded with the shortest distance to accept, which equivalent states share: a counting chain
    # {m,n} is then split at once instead of one state per round)
    live = sorted(good)
    dist = {q: 0 for q in live if acc[q]}
    todo = list(dist)
    while todo:
        nxt_todo = []
        for t in todo:
            for p in rev[t]:
                if p not in dist:
                    dist[p] = dist[t] + 1
                    nxt_todo.append(p)
        todo = nxt_todo
    seed: Dict[int, int] = {}
    block = {q: seed.setdefault(dist[q], len(seed)) for q in live}
    while True:
        keys: Dict[tuple, int] = {}
        nxt = {}
        for q in live:
            row = drows[q]
            kk = (block[q], tuple(block.get(row.get(c, -1), -1) for c in range(ncls)))
            nxt[q] = keys.setdefault(kk, len(keys))
        stable = len(keys) == len(set(block.values()))
        block = nxt
        if stable:
            break
    nb = len(set(block.values()))
    rows: List[Dict[int, Tuple[int, int]]] = [dict() for _ in range(nb)]
    accept = [False] * nb
    done = set()
    for q in live:
        bq = block[q]
        accept[bq] = accept[bq] or acc[q]
        if bq in done:
            continue
        done.add(bq)
        row = drows[q]
        for byte in range(256):
            t = row.get(bcls[byte])
            if t is not None and t in block:
                rows[bq][byte] = (block[t], ACT_NONE)
    return _finish(kind, key, rows, accept, block[0])


# ---- json_schema -> AST ---------------------------------------------------------------------------------

_SWS = ("rep", ("set", _mask(b" \n\t")), 0, None)        # whitespace between tokens: [ \n\t]*
_ANNOTATIONS = {"title", "description", "$schema", "$id", "$comment", "default", "examples"}
_INT_AST = ("cat", [("rep", ("set", 1 << 0x2D), 0, 1),
                    ("alt", [("set", 1 << 0x30), ("cat", [("set", _mask(b"123456789")),
                                                          ("rep", ("set", _mask(_DIGITS)), 0, None)])])])
_NUM_AST = ("cat", [_INT_AST,
                    ("rep", ("cat", [("set", 1 << 0x2E), ("rep", ("set", _mask(_DIGITS)), 1, None)]), 0, 1),
                    ("rep", ("cat", [("set", _mask(b"eE")), ("rep", ("set", _mask(b"+-")), 0, 1),
                                     ("rep", ("set", _mask(_DIGITS)), 1, None)]), 0, 1)])


def _string_char():
    """One character of a schema string, for minLength / maxLength: a code point, a short escape, a
    ``\\uXXXX`` escape outside the surrogates, or an escaped surrogate PAIR (one character). Lone
    escaped surrogates are not accepted here (json_object accepts them)."""
    plain = cp_class([(0x20, 0x21), (0x23, 0x5B), (0x5D, _MAX_CP)])
    hx = ("set", _mask(_HEX))
    d, u = ("set", _mask(b"dD")), lit(b"\\u")
    bmp = ("cat", [("set", 1 << 0x75), ("alt", [("cat", [("set", _mask(_HEX) & ~_mask(b"dD")), ("rep", hx, 3, 3)]),
                                                ("cat", [d, ("set", _mask(b"01234567")), ("rep", hx, 2, 2)])])])
    pair = ("cat", [("set", 1 << 0x75), d, ("set", _mask(b"89abAB")), ("rep", hx, 2, 2),
                    u, d, ("set", _mask(b"cdefCDEF")), ("rep", hx, 2, 2)])
    esc = ("cat", [("set", 1 << 0x5C), ("alt", [("set", _mask(b'"\\/bfnrt')), bmp, pair])])
    return ("alt", [plain, esc])


def _scalar_lit(v, where: str):
    if isinstance(v, (dict, list)):
        raise ValueError(f"json_schema: {where} supports scalars only")
    return lit(json.dumps(v, ensure_ascii=False).encode("utf-8"))


def _check_keys(schema: dict, allowed: set) -> None:
    for k in schema:
        if k not in allowed and k not in _ANNOTATIONS:
            raise ValueError(f"json_schema: unsupported keyword {k!r}")


def _nonneg(schema: dict, k: str, default):
    v = schema.get(k, default)
    if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 0):
        raise ValueError(f"json_schema: {k} must be a non-negative integer")
    return v


def schema_to_ast(schema):
    """Supported: ``type`` object with ``properties`` (emitted in listed order, all present; ``required``
    must name all of them; ``additionalProperties`` only ``false``), nested objects, ``array`` with
    ``items`` / ``minItems`` / ``maxItems``, ``string`` with ``minLength`` / ``maxLength`` (code points)
    / ``enum``, ``integer``, ``number``, ``boolean``, ``null``, ``enum`` / ``const`` of scalars,
    ``anyOf``. Any other keyword raises ValueError naming it; recursion (``$ref``) is not supported."""
    if not isinstance(schema, dict):
        raise ValueError("json_schema: a schema must be an object")
    if "anyOf" in schema:
        _check_keys(schema, {"anyOf"})
        alts = schema["anyOf"]
        if not isinstance(alts, list) or not alts:
            raise ValueError("json_schema: anyOf must be a non-empty list")
        return ("alt", [schema_to_ast(a) for a in alts])
    if "const" in schema:
        _check_keys(schema, {"const", "type"})
        return _scalar_lit(schema["const"], "const")
    if "enum" in schema:
        _check_keys(schema, {"enum", "type"})
        vals = schema["enum"]
        if not isinstance(vals, list) or not vals:
            raise ValueError("json_schema: enum must be a non-empty list")
        return ("alt", [_scalar_lit(v, "enum") for v in vals])
    t = schema.get("type")
    if t == "object":
        _check_keys(schema, {"type", "properties", "required", "additionalProperties"})
        props = schema.get("properties", {})
        if not isinstance(props, dict):
            raise ValueError("json_schema: properties must be an object")
        if schema.get("additionalProperties", False) is not False:
            raise ValueError("json_schema: unsupported keyword 'additionalProperties' (only false)")
        if "required" in schema and set(schema["required"]) != set(props):
            raise ValueError("json_schema: 'required' must name every property (all listed properties are emitted)")
        items = [("set", 1 << 0x7B), _SWS]
        for i, (name, sub) in enumerate(props.items()):
            if i:
                items += [("set", 1 << 0x2C), _SWS]
            items += [lit(json.dumps(name, ensure_ascii=False).encode("utf-8")), _SWS, ("set", 1 << 0x3A), _SWS,
                      schema_to_ast(sub), _SWS]
        items.append(("set", 1 << 0x7D))
        return ("cat", items)
    if t == "array":
        _check_keys(schema, {"type", "items", "minItems", "maxItems"})
        if "items" not in schema:
            raise ValueError("json_schema: an array needs 'items'")
        item = schema_to_ast(schema["items"])
        lo, hi = _nonneg(schema, "minItems", 0), _nonneg(schema, "maxItems", None)
        if hi is not None and hi < lo:
            raise ValueError("json_schema: maxItems < minItems")
        if max(lo, hi or 0) > _REP_MAX:
            raise ValueError(f"json_schema: minItems / maxItems above {_REP_MAX}")
        more = ("cat", [_SWS, ("set", 1 << 0x2C), _SWS, item])
        body = ("cat", [item, ("rep", more, max(lo - 1, 0), None if hi is None else hi - 1)])
        if hi == 0:
            body = ("cat", [])
        elif lo == 0:
            body = ("rep", body, 0, 1)
        return ("cat", [("set", 1 << 0x5B), _SWS, body, _SWS, ("set", 1 << 0x5D)])
    if t == "string":
        _check_keys(schema, {"type", "minLength", "maxLength"})
        lo, hi = _nonneg(schema, "minLength", 0), _nonneg(schema, "maxLength", None)
        if hi is not None and hi < lo:
            raise ValueError("json_schema: maxLength < minLength")
        if max(lo, hi or 0) > _REP_MAX:
            raise ValueError(f"json_schema: minLength / maxLength above {_REP_MAX}")
        q = ("set", 1 << 0x22)
        return ("cat", [q, ("rep", _string_char(), lo, hi), q])
    if t in ("integer", "number", "boolean", "null"):
        _check_keys(schema, {"type"})
        return {"integer": _INT_AST, "number": _NUM_AST, "null": lit(b"null"),
                "boolean": ("alt", [lit(b"true"), lit(b"false")])}[t]
    if "type" not in schema:
        for k in schema:
            if k not in _ANNOTATIONS:
                raise ValueError(f"json_schema: unsupported keyword {k!r}")
        raise ValueError("json_schema: a schema needs 'type', 'enum', 'const' or 'anyOf'")
    raise ValueError(f"json_schema: unsupported type {t!r}")


# ---- the public compiler --------------------------------------------------------------------------------

def canonical_spec(spec) -> str:
    """The cache key of a grammar spec. Key order is kept: a schema's properties are emitted in it."""
    if not isinstance(spec, dict) or not isinstance(spec.get("type"), str):
        raise ValueError('grammar must be {"type": "json_object" | "json_schema" | "regex", ...}')
    t = spec["type"]
    want = {"json_object": {"type"}, "json_schema": {"type", "schema"}, "regex": {"type", "pattern"},
            "tail": {"type", "open", "body", "close"}}.get(t)
    if want is None:
        raise ValueError(f"unknown grammar type {t!r}")
    if set(spec) != want:
        raise ValueError(f"a {t} grammar takes exactly the fields {sorted(want)}")
    if t == "tail":
        for k, lo in (("open", 1), ("close", 0)):
            v = spec[k]
            if not isinstance(v, str) or not lo <= len(v.encode("utf-8")) <= TAIL_MAX_BYTES:
                raise ValueError(f"a tail grammar's {k!r} must be a string of {lo}..{TAIL_MAX_BYTES} bytes")
        body = spec["body"]
        if not isinstance(body, dict) or body.get("type") not in ("json_schema", "regex"):
            raise ValueError("a tail grammar's 'body' must be a json_schema or regex grammar")
        canonical_spec(body)
    try:
        return json.dumps(spec, ensure_ascii=False, allow_nan=False)
    except (TypeError, ValueError) as e:
        raise ValueError(f"grammar is not JSON: {e}") from None


@functools.lru_cache(maxsize=256)
def _compile(key: str) -> CompiledGrammar:
    spec = json.loads(key)
    t = spec["type"]
    if t == "json_object":
        return _build_json(key)
    if t == "regex":
        return _ast_to_grammar("regex", key, parse_regex(spec["pattern"]))
    if t == "tail":
        body = spec["body"]
        ast = parse_regex(body["pattern"]) if body["type"] == "regex" else schema_to_ast(body["schema"])
        return _ast_to_grammar("tail", key, ("cat", [ast, lit(spec["close"].encode("utf-8"))]),
                               opener=spec["open"].encode("utf-8"))
    return _ast_to_grammar("json_schema", key, schema_to_ast(spec["schema"]))


def compile_grammar(spec) -> CompiledGrammar:
    """ValueError for a bad spec, an unsupported construct or a grammar over the caps. Cached."""
    return _compile(canonical_spec(spec))


# ---- token bytes ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _bytelevel_inverse() -> Dict[str, int]:
    """The inverse of the byte-level BPE alphabet (every byte shown as a printable character)."""
    keep = list(range(0x21, 0x7F)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    inv, n = {}, 0
    for b in range(256):
        if b in keep:
            inv[chr(b)] = b
        else:
            inv[chr(256 + n)] = b
            n += 1
    return inv


class TokenTable:
    """Bytes of every token id in ``[0, vocab)``: ``pieces[i]`` (``b""`` for special / added tokens and
    ids the tokenizer does not know: never allowed under a grammar, except stop ids) and the stop ids."""

    def __init__(self, pieces: Sequence[bytes], stop_ids: Iterable[int], name: str = "tokens"):
        self.pieces = list(pieces)
        self.vocab = len(self.pieces)
        self.stop_ids = tuple(sorted({int(i) for i in stop_ids if 0 <= int(i) < self.vocab}))
        if not self.stop_ids:
            raise ValueError("a grammar needs a stop id inside the vocabulary")
        if len(self.stop_ids) > GRAMMAR_MAX_STOPS:
            raise ValueError(f"at most {GRAMMAR_MAX_STOPS} stop ids are supported under a grammar")
        for i in self.stop_ids:
            self.pieces[i] = b""
        self.name = name
        # shortest first: the binding check stops at the first token a state allows
        self.by_len = sorted((i for i, p in enumerate(self.pieces) if 0 < len(p) <= GRAMMAR_TOKEN_BYTE_CAP),
                             key=lambda i: len(self.pieces[i]))
        self._dev: dict = {}

    def tensors(self, device=None):
        """``(tok_off int32[V + 1], tok_bytes uint8[N])`` on ``device`` (cached). N is padded to a positive
        multiple of 16: the kernel fetches token bytes 16 at a time."""
        import torch
        key = str(device)
        if key not in self._dev:
            off = [0]
            for p in self.pieces:
                off.append(off[-1] + len(p))
            data = b"".join(self.pieces)
            data += bytes(16 - len(data) % 16)
            self._dev[key] = (torch.tensor(off, dtype=torch.int32).to(device),
                              torch.frombuffer(bytearray(data), dtype=torch.uint8).clone().to(device))
        return self._dev[key]


def _added_ids(tok) -> set:
    try:
        return {int(i) for i in tok.get_added_tokens_decoder()}
    except AttributeError:      # older `tokenizers`
        return {int(a["id"]) for a in json.loads(tok.to_str()).get("added_tokens", [])}


def token_table(tokenizer, vocab: int) -> TokenTable:
    """The token byte table of an :class:`EngineTokenizer` or :class:`HFTokenizer` for a model with
    ``vocab`` logits, cached on the tokenizer. ValueError for a tokenizer whose vocabulary is neither
    byte-level nor Metaspace with ``<0xNN>`` byte fallback."""
    cache = tokenizer.__dict__.setdefault("_grammar_tables", {})
    if vocab in cache:
        return cache[vocab]
    from .tokenizer import EngineTokenizer, _fallback_piece
    tok = getattr(tokenizer, "_tok", None)
    if tok is None:
        raise ValueError(f"tokenizer {getattr(tokenizer, 'name', tokenizer)!r} has no vocabulary to bind a grammar to")
    spec = json.loads(tok.to_str())
    kinds = set()
    for part in (spec.get("pre_tokenizer"), spec.get("decoder")):
        todo = [part]
        while todo:
            p = todo.pop()
            if isinstance(p, dict):
                kinds.add(p.get("type"))
                todo += list(p.get("pretokenizers", [])) + list(p.get("decoders", []))
    words = tok.get_vocab(with_added_tokens=True)
    added = _added_ids(tok)
    pieces = [b""] * vocab
    if "ByteLevel" in kinds:
        inv = _bytelevel_inverse()
        for w, i in words.items():
            if i < vocab and i not in added:
                try:
                    pieces[i] = bytes(inv[ch] for ch in w)
                except KeyError:
                    pieces[i] = b""
    elif any(f"<0x{b:02X}>" in words for b in (0x22, 0x7B)) and ("Metaspace" in kinds or any("▁" in w for w in words)):
        for w, i in words.items():
            if i >= vocab or i in added:
                continue
            if len(w) == 6 and w.startswith("<0x") and w.endswith(">"):
                try:
                    pieces[i] = bytes([int(w[3:5], 16)])
                    continue
                except ValueError:
                    pass
            pieces[i] = w.replace("▁", " ").encode("utf-8")
    else:
        raise ValueError(f"tokenizer {getattr(tokenizer, 'name', '?')!r} is neither byte-level nor Metaspace with "
                         f"byte fallback: a grammar cannot be bound to it")
    if isinstance(tokenizer, EngineTokenizer):
        for i in range(tokenizer.base_vocab, vocab):     # ids the BPE does not know decode to printable pieces
            pieces[i] = _fallback_piece(i).encode("utf-8")
    cache[vocab] = TokenTable(pieces, tokenizer.stop_ids, getattr(tokenizer, "name", "tokens"))
    return cache[vocab]


# ---- a grammar bound to a token table -------------------------------------------------------------------

class BoundGrammar:
    """A compiled grammar and a token table that passed the pairing check: every state ``q`` allows at
    least one token at ``depth = 0`` and at ``depth = GRAMMAR_MAX_DEPTH`` (a stop id where ``q``
    accepts), and some sequence of tokens leads from ``q`` to an accepting state. With the ``DEAD``
    rule the first is why no row's logits can become all ``-inf``."""

    def __init__(self, g: CompiledGrammar, table: TokenTable, check: bool = True):
        """``check=False`` skips the pairing check: only for exercising the mask at arbitrary states over
        a synthetic table (the engine always checks, through :func:`bind`)."""
        self.g, self.table = g, table
        self._stops = frozenset(table.stop_ids)
        if not check:
            return
        full = (1 << GRAMMAR_MAX_DEPTH) - 1
        shapes = [(0, 0), (GRAMMAR_MAX_DEPTH, 0), (GRAMMAR_MAX_DEPTH, full)] if g.uses_stack else [(0, 0)]
        for q in range(g.n_states):
            if g.accept[q]:
                continue
            for depth, stack in shapes:
                if not any(g.walk((q, depth, stack), table.pieces[i])[0] >= 0 for i in table.by_len):
                    raise ValueError(f"the {g.kind} grammar cannot be bound to tokenizer {table.name!r}: no token "
                                     f"continues state {q} at depth {depth}")
        self._check_progress()

    def _abstract_walk(self, q: int, data: bytes) -> set:
        """The states ``data`` can lead to from ``q`` on SOME stack (a pop goes to every pop target)."""
        g = self.g
        pops = [p for p in g.pop_target if p >= 0]
        cur = {q}
        for byte in data:
            nxt = set()
            for s in cur:
                e = g.trans[s * g.n_classes + g.cls[byte]]
                if e != DEAD_ENTRY:
                    nxt.update(pops) if (e & 3) == ACT_POP else nxt.add(e >> 2)
            cur = nxt
            if not cur:
                break
        return cur

    def _check_progress(self) -> None:
        """Beyond "some token is allowed": from every state some sequence of TOKENS reaches an accepting
        state (on some stack). A vocabulary without the byte ``"`` passes the first check in the state
        after a comma in an object, where whitespace is allowed, but can never write the next key."""
        g, table = self.g, self.table
        n, ncls = g.n_states, g.n_classes
        pops = [p for p in g.pop_target if p >= 0]
        single = sorted({g.cls[p[0]] for p in table.pieces if len(p) == 1})
        rev: List[List[int]] = [[] for _ in range(n)]
        for q in range(n):
            for c in single:
                e = g.trans[q * ncls + c]
                if e != DEAD_ENTRY:
                    for t in (pops if (e & 3) == ACT_POP else [e >> 2]):
                        rev[t].append(q)
        good = {q for q in range(n) if g.accept[q]}

        def spread(todo: List[int]) -> None:
            while todo:
                for p in rev[todo.pop()]:
                    if p not in good:
                        good.add(p)
                        todo.append(p)

        spread(list(good))
        rest = [q for q in range(n) if q not in good]
        multi = [i for i in table.by_len if len(table.pieces[i]) > 1]
        changed = True
        while rest and changed:       # states only longer tokens can leave (none with a byte-level vocabulary)
            changed = False
            for q in rest:
                if q not in good and any(self._abstract_walk(q, table.pieces[i]) & good for i in multi):
                    good.add(q)
                    spread([q])
                    changed = True
            rest = [q for q in rest if q not in good]
        if rest:
            raise ValueError(f"the {g.kind} grammar cannot be bound to tokenizer {table.name!r}: no sequence of "
                             f"tokens completes state {rest[0]}")

    def token_allowed(self, state: State, tok: int) -> bool:
        if tok in self._stops:
            return state[0] < 0 or self.g.is_accepting(state)
        if state[0] < 0 or not 0 <= tok < self.table.vocab:
            return False
        p = self.table.pieces[tok]
        return 0 < len(p) <= GRAMMAR_TOKEN_BYTE_CAP and self.g.walk(state, p)[0] >= 0

    def advance(self, state: State, tok: int) -> State:
        """The state after consuming token ``tok``: a stop id gives ``FIN``; a token that is not allowed
        gives ``DEAD``; ``FIN`` and ``DEAD`` stay."""
        if state[0] < 0:
            return state
        if tok in self._stops:
            return FIN
        if not 0 <= tok < self.table.vocab:
            return DEAD
        p = self.table.pieces[tok]
        if not 0 < len(p) <= GRAMMAR_TOKEN_BYTE_CAP:
            return DEAD
        return self.g.walk(state, p)

    def state_after(self, tokens: Iterable[int], state: Optional[State] = None) -> State:
        st = self.g.start_state if state is None else state
        for t in tokens:
            st = self.advance(st, int(t))
        return st

    def budget(self) -> "GrammarBudget":
        """The pair's :class:`GrammarBudget` (cached). ValueError when a state can only be left by
        multi-byte tokens: the bound on the tokens a document still needs rests on single-byte ones."""
        b = self.__dict__.get("_budget")
        if b is None:
            b = self._budget = GrammarBudget(self)
        return b

    def all_live(self) -> bytes:
        """Per state: every token with usable bytes stays live from it (cached; :class:`GrammarBudget`)."""
        f = self.__dict__.get("_all_live")
        if f is None:
            f = self._all_live = GrammarBudget._all_live(self.g, self.table)
        return f

    def token_allowed_budget(self, state: State, tok: int, r: int) -> bool:
        """:meth:`token_allowed` under the budget rule (:class:`GrammarBudget`), ``r`` tokens left."""
        if tok in self._stops:      # r <= 0 behaves like DEAD: stop ids only
            return r <= 0 or state[0] < 0 or self.g.is_accepting(state)
        return r > 0 and self.token_allowed(state, tok) and self.budget().need(self.advance(state, tok)) <= r - 2


class GrammarBudget:
    """What the budgeted mask (csrc/grammar_budget.hip) reads beside the automaton, for one bound pair.

    ``need(state)`` is an upper bound on the tokens that still lead from ``state`` to an accepting
    state, along byte classes that have a single-byte token (so every step of that path is one token
    whatever the stack holds):

    * ``c_pop[q]``: the fewest such tokens up to and including the next pop, over edges without an
      action (a push is never needed to close what is open);
    * ``c_acc[q]``, for depth 0: the fewest tokens to an accepting state, where a push edge to ``t``
      costs ``1 + c_pop[t] + c_acc0[pop_empty]`` (``c_acc0``: the same without push edges);
    * ``need = c_acc[q]`` at depth 0, else ``c_pop[q]`` + one ``c_pop[pop_target[bit]]`` per stack level
      below the top + ``c_acc[pop_empty]``: two popcounts.

    The first token of the path that defines ``need`` lowers it by at least one. So with ``r`` tokens
    left (the one sampled now included) and the rule "a non-stop token is allowed iff its walk stays
    live and ``need(state after it) <= r - 2``", ``need(state) <= r - 1`` holds at every step once it holds
    at the start; some token is always allowed; and at ``r = 1`` the state accepts, so the stop id ends
    the reply inside the budget. Entries are 16-bit, ``NEED_INF16`` for none.

    ``all_live[q]``: every token with usable bytes stays live from ``q`` (the free states of a ``tail``
    grammar; a token that holds the whole opener and then a bad byte clears it). ``need_cap``: the
    largest ``need`` of a regular grammar; in a flagged state with ``r - 2 >= need_cap`` the rule allows
    every token with bytes, and the kernel walks none."""

    def __init__(self, bound: "BoundGrammar"):
        import heapq
        g, table = bound.g, bound.table
        n, ncls = g.n_states, g.n_classes
        single = sorted({g.cls[p[0]] for p in table.pieces if len(p) == 1})
        inf = NEED_INF
        rev: List[List[int]] = [[] for _ in range(n)]          # edges without an action, reversed
        pushes: List[Tuple[int, int]] = []
        c_pop = [inf] * n
        for q in range(n):
            for c in single:
                e = g.trans[q * ncls + c]
                if e == DEAD_ENTRY:
                    continue
                if (e & 3) == ACT_POP:
                    c_pop[q] = 1
                elif e & 3:
                    pushes.append((q, e >> 2))
                else:
                    rev[e >> 2].append(q)

        def spread(cost: List[int]) -> List[int]:
            """Shortest costs to the seeded states over the unit edges of ``rev``."""
            heap = [(c, q) for q, c in enumerate(cost) if c < inf]
            heapq.heapify(heap)
            while heap:
                c, q = heapq.heappop(heap)
                if c > cost[q]:
                    continue
                for p in rev[q]:
                    if c + 1 < cost[p]:
                        cost[p] = c + 1
                        heapq.heappush(heap, (c + 1, p))
            return cost

        c_pop = spread(c_pop)
        seed = [0 if a else inf for a in g.accept]
        c_acc = spread(list(seed))
        pe = g.pop_target[2]
        if g.uses_stack and pe >= 0 and c_acc[pe] < inf:
            for q, t in pushes:        # a push at depth 0: its container closes, then pop_empty's way to accept
                seed[q] = min(seed[q], 1 + c_pop[t] + c_acc[pe])
            c_acc = spread(seed)
        bad = [q for q in range(n) if min(c_acc[q], c_pop[q] if g.uses_stack else inf) >= NEED_INF16]
        if g.uses_stack:
            bad += [p for p, c in zip(g.pop_target, (c_pop, c_pop, c_acc)) if p >= 0 and c[p] >= NEED_INF16]
        if bad:
            raise ValueError(f"the {g.kind} grammar cannot finish inside a budget with tokenizer {table.name!r}: "
                             f"state {bad[0]} can only be left by multi-byte tokens")
        self.g = g
        self.c_acc = [min(c, NEED_INF16) for c in c_acc]
        self.c_pop = [min(c, NEED_INF16) for c in c_pop]
        self.need_cap = NEED_INF if g.uses_stack else max(self.c_acc)
        self.all_live = bound.all_live()
        self.need_start = self.need(g.start_state)

    def need(self, state: State) -> int:
        """csrc/grammar_core.h ``need``. 0 for ``FIN`` / ``DEAD``: only stop ids follow."""
        q, depth, stack = state
        if q < 0:
            return 0
        pobj, parr, pempty = self.g.pop_target
        if depth == 0:
            parts = [(self.c_acc[q], 1)]
        else:
            ones = bin(stack & ((1 << (depth - 1)) - 1)).count("1")
            parts = [(self.c_pop[q], 1), (self.c_pop[pobj] if pobj >= 0 else NEED_INF16, depth - 1 - ones),
                     (self.c_pop[parr] if parr >= 0 else NEED_INF16, ones),
                     (self.c_acc[pempty] if pempty >= 0 else NEED_INF16, 1)]
        if any(c == NEED_INF16 and k for c, k in parts):
            return NEED_INF
        return sum(c * k for c, k in parts)

    def min_tokens(self) -> int:
        """The smallest ``max_new_tokens`` the rule can start from: ``need(start)`` and the stop id."""
        return self.need_start + 1

    @staticmethod
    def _all_live(g: CompiledGrammar, table: TokenTable) -> bytes:
        ids = table.by_len
        n, ncls = g.n_states, g.n_classes
        flags = bytearray(n)
        if g.uses_stack or not ids:
            return bytes(flags)
        firsts = sorted({g.cls[table.pieces[i][0]] for i in ids})
        cand = [q for q in range(n) if all(g.trans[q * ncls + c] != DEAD_ENTRY for c in firsts)]
        if not cand:
            return bytes(flags)
        import torch       # every token walked at once, one byte position per iteration
        lens = torch.tensor([len(table.pieces[i]) for i in ids], dtype=torch.int64)       # ascending
        off = torch.cumsum(lens, 0) - lens
        flat = torch.frombuffer(bytearray(b"".join(table.pieces[i] for i in ids)), dtype=torch.uint8).long()
        cls = torch.tensor(list(g.cls), dtype=torch.int64)[flat]
        trans = torch.tensor(g.trans, dtype=torch.int64)
        for q0 in cand:
            q = torch.full((len(ids),), q0, dtype=torch.int64)
            ok = True
            for p in range(int(lens[-1])):
                lo = int(torch.searchsorted(lens, p, right=True))      # tokens longer than p
                e = trans[q[lo:] * ncls + cls[off[lo:] + p]]
                if bool((e == DEAD_ENTRY).any()):
                    ok = False
                    break
                q[lo:] = e >> 2
            flags[q0] = 1 if ok else 0
        return bytes(flags)


def bind(spec, tokenizer, vocab: int) -> BoundGrammar:
    """Compile ``spec`` and bind it to ``tokenizer`` (cached on the token table). ValueError if either fails."""
    table = token_table(tokenizer, vocab)
    g = compile_grammar(spec)
    cache = table.__dict__.setdefault("_bound", {})       # least recently used first; as many as _compile keeps
    bound = cache.pop(g.key, None)
    if bound is None or bound.g is not g:
        bound = BoundGrammar(g, table)
    cache[g.key] = bound
    while len(cache) > _BOUND_CACHE:
        cache.pop(next(iter(cache)))
    return bound
