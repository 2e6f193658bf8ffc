"""The grammar mask's host-visible code under AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU:
csrc/tests/grammar_check.cpp (its own ``main``; nothing is preloaded) runs the walk of
csrc/grammar_core.h — the copy the kernel runs — against the Python walker, the refusals of
``plan_grammar_mask`` and the launcher's argument validation, which rejects before any HIP call.

The case file is whitespace-separated integers: ``n_states n_classes pop_obj pop_arr pop_empty``, 256 class
ids, the table, ``n_stop`` and the stop ids, ``V`` and ``V + 1`` token offsets, the byte count and the
bytes; then the cases ``kind q depth stack`` + (kind 0: ``n`` and n bytes | kind 1: a token id) + the
expected ``q depth stack``; then the plans: 15 arguments of ``plan_grammar_mask`` + the expected rc and chunks."""
import os
import random
import shutil
import subprocess

import pytest

from theroundtaible_amd.engine import grammar as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
CAP, BYTE_CAP = G.GRAMMAR_MAX_DEPTH, G.GRAMMAR_TOKEN_BYTE_CAP
JSON = G.compile_grammar({"type": "json_object"})
DOCS = [b'{"a":[1,-2.5e+3,true,false,null,{"b":"c\\n\\u00e9"}],"d":{}}', '{"é€😀":"x"}'.encode(), b' {\n"k" : [ [ ] , { } ] }',
        b'{"a":' * CAP + b"1" + b"}" * CAP, b'{"a":' + b"[" * (CAP - 1) + b"]" * (CAP - 1) + b"}"]


def cases():
    rng = random.Random(4)
    pieces = [b"", b"", b"x" * BYTE_CAP, b"x" * (BYTE_CAP + 1), b'{"', b'"}', b"[[[", b"]]]", b"}]}", b'":[{"k":', b"1"]
    pieces += [bytes([b]) for b in range(256)]
    table = G.TokenTable(pieces, [1])
    bound = G.BoundGrammar(JSON, table, check=False)
    out = []

    def walk(st, data, want=None):
        want = JSON.walk(st, data) if want is None else want
        out.append([0, *st, len(data), *data, *want])

    def advance(st, tok, want=None):
        want = bound.advance(st, tok) if want is None else want
        out.append([1, *st, tok, *want])

    start = JSON.start_state
    for doc in DOCS:
        assert JSON.accepts(doc)
        walk(start, doc)
        for _ in range(12):                                 # from a state mid-document over a slice, whole or mutated
            i = rng.randrange(len(doc))
            j = rng.randrange(i, len(doc) + 1)
            data = bytearray(doc[i:j])
            if data and rng.random() < 0.5:
                data[rng.randrange(len(data))] = rng.choice(b'{}[]":,\\ 1e.-x\x80\xc3\xff')
            walk(JSON.walk(start, doc[:i]), bytes(data))
    at_cap = JSON.walk(start, b'{"a":' * CAP)
    assert at_cap[1] == CAP
    walk(at_cap, b"{", G.DEAD)                              # a push at the depth cap
    walk(at_cap, b"[", G.DEAD)
    walk(at_cap, b"1" + b"}" * CAP)                         # and all the way down
    walk(start, b"}", G.DEAD)                               # a pop on an empty stack
    walk((JSON.names["after_obj"], 0, 0), b"}", G.DEAD)
    walk((JSON.names["after_arr"], 1, 1), b"]")             # the last pop: to pop_target[empty]
    walk(start, b"")                                        # zero bytes
    walk(G.FIN, b"{", G.FIN)
    walk(G.DEAD, b"{", G.DEAD)
    # indices at the table's edge: the last state, the bytes of the last class, a state one past the table
    last_cls = [b for b in range(256) if JSON.cls[b] == JSON.n_classes - 1]
    for byte in (last_cls[0], last_cls[-1], 0, 255):
        walk((JSON.n_states - 1, 1, 0), bytes([byte]))
        walk((0, 0, 0), bytes([byte]))
    walk((JSON.n_states, 0, 0), b"{", G.DEAD)
    walk((5, CAP + 1, 0), b" ", G.DEAD)
    walk((5, -1, 0), b" ", G.DEAD)
    in_string = JSON.walk(start, b'{"a')
    for tok in range(len(pieces)):
        advance(in_string, tok)
    for st in (start, JSON.walk(start, b'{"a":[{"k":[['), JSON.walk(start, b"{}"), at_cap, G.FIN, G.DEAD):
        for tok in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, len(pieces) - 1, len(pieces), -1, 1 << 40):
            advance(st, tok)
    assert bound.advance(in_string, 0) == G.DEAD and bound.advance(in_string, 1) == G.FIN      # zero bytes; a stop id
    assert bound.advance(in_string, 2)[0] >= 0 and bound.advance(in_string, 3) == G.DEAD       # at the cap; over it
    return table, out


T, S, C, M = G.GRAMMAR_MAX_TABLE, G.GRAMMAR_MAX_STATES, G.GRAMMAR_MAX_CLASSES, 128256
OK = [3, M, M, 0, T, S, C, BYTE_CAP, M + 1, 1008, 3, 0, 0, 0, 0]
# B V ld dtype tab_entries state_cap classes_cap byte_cap n_off n_bytes rows has_out has_step max_steps out_ld -> rc, chunks
# (chunks: workgroups per row, 256 ids each)


def plan(rc, chunks=0, **kw):
    names = ["B", "V", "ld", "dtype", "tab", "states", "classes", "byte_cap", "n_off", "n_bytes", "rows", "has_out",
             "has_step", "max_steps", "out_ld"]
    a = list(OK)
    for k, v in kw.items():
        a[names.index(k)] = v
    return a + [rc, chunks]


PLANS = [
    plan(0, 501), plan(0, 501, dtype=1, ld=M + 8), plan(0, 1, V=33, ld=33), plan(0, 1, V=256, ld=256),
    plan(0, 2, V=257, ld=257), plan(0, 17, V=4099, ld=4104), plan(0, 4096, V=1 << 20, ld=1 << 20, n_off=(1 << 20) + 1),
    plan(0, 501, has_out=1, has_step=1, max_steps=8192, out_ld=3), plan(0, 501, has_out=1, has_step=1, max_steps=0, out_ld=8),
    plan(0, 501, tab=8, states=1, classes=1), plan(0, 501, rows=64),
    plan(-1, V=0), plan(-1, V=-5), plan(-1, ld=M - 1), plan(-2, V=(1 << 20) + 1, ld=1 << 21, n_off=1 << 22),
    plan(-3, dtype=2), plan(-3, dtype=-1), plan(-4, tab=T + 8), plan(-4, tab=0), plan(-4, tab=12), plan(-4, states=S + 1),
    plan(-4, states=0), plan(-5, classes=C + 1), plan(-5, classes=0), plan(-6, byte_cap=BYTE_CAP + 1), plan(-6, byte_cap=64),
    plan(-7, has_out=1), plan(-7, has_step=1), plan(-8, has_out=1, has_step=1, out_ld=2), plan(-8, has_out=1, has_step=1,
                                                                                                 out_ld=3, max_steps=-1),
    plan(-9, n_off=M), plan(-9, n_bytes=0), plan(-9, n_bytes=1000), plan(-9, n_bytes=8), plan(0, 501, n_bytes=16),
    plan(-10, rows=2),
]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_walk_plan_and_launcher_under_asan_ubsan(tmp_path):
    table, rows = cases()
    off = [0]
    for p in table.pieces:
        off.append(off[-1] + len(p))
    data = b"".join(table.pieces)
    nums = [JSON.n_states, JSON.n_classes, *JSON.pop_target, *JSON.cls, *JSON.trans, len(table.stop_ids), *table.stop_ids,
            table.vocab, *off, len(data), *data, len(rows)]
    for r in rows:
        nums += r
    nums.append(len(PLANS))
    for p in PLANS:
        nums += p
    path = tmp_path / "cases.txt"
    path.write_text(" ".join(str(int(n)) for n in nums))
    exe = str(tmp_path / "grammar_check")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(CSRC, "tests", "grammar_check.cpp"), os.path.join(CSRC, "grammar_mask.hip"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    nm = shutil.which("nm")
    if nm:
        syms = subprocess.run([nm, exe], capture_output=True, text=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms   # the sanitizers really are linked in
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "0 failure(s)" in r.stdout and len(rows) > 400
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
