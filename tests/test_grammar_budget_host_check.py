"""The budgeted grammar mask's host-visible code under AddressSanitizer + UndefinedBehaviorSanitizer, without a
GPU: csrc/tests/grammar_budget_check.cpp (its own ``main``; nothing is preloaded) runs ``need``, ``remaining``,
``budget_allows`` and ``walks_skippable`` of csrc/grammar_core.h — the copies the kernel runs — against
``engine.grammar.GrammarBudget`` and the rule as the Python side states it, the refusals of
``plan_grammar_budget`` and the launcher's argument validation, which rejects before any HIP call.

The case file is whitespace-separated integers: the number of grammars; per grammar ``n_states pop_obj
pop_arr pop_empty``, ``c_acc`` and ``c_pop`` (n_states entries each), the number of cases and per case ``q
depth stack`` + the expected need; then the rules ``budget step need_after all_live need_cap`` + the
expected ``r allows skippable``; then the plans: 18 arguments of ``plan_grammar_budget`` + the expected rc
and chunks."""
import os
import random
import shutil
import subprocess

import pytest

from test_grammar_cpu import FINITE
from test_grammar_host_check import BYTE_CAP, OK, C, M, S, T
from theroundtaible_amd.engine import grammar as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
CAP = G.GRAMMAR_MAX_DEPTH


def need_cases():
    rng = random.Random(5)
    table = G.TokenTable([b""] + [bytes([b]) for b in range(256)] + [b'{"', b"]]"], [0])
    out = []
    for spec in ({"type": "json_object"}, {"type": "json_schema", "schema": FINITE},
                 {"type": "tail", "open": "ab", "body": {"type": "regex", "pattern": "x{3,}y?"}, "close": "\n"}):
        g = G.compile_grammar(spec)
        bd = G.BoundGrammar(g, table).budget()
        cases = []
        for q in range(g.n_states):
            cases.append((q, 0, 0, bd.need((q, 0, 0))))
            if g.uses_stack:
                for depth in (1, 2, 3, 17, CAP - 1, CAP):
                    for stack in (0, (1 << depth) - 1, rng.getrandbits(depth), rng.getrandbits(32)):
                        cases.append((q, depth, stack, bd.need((q, depth, stack))))
        # outside the table: never an index into the arrays
        cases += [(g.n_states, 0, 0, G.NEED_INF), (-1, 0, 0, G.NEED_INF), (0, -1, 0, G.NEED_INF), (0, CAP + 1, 0, G.NEED_INF)]
        out.append((g, bd, cases))
    # entries that say "none": at depth 0, at the pop targets, in c_pop[q]
    g, bd, _ = out[0]
    for kill in ("acc", "pop", "obj", "empty"):
        acc, pop = list(bd.c_acc), list(bd.c_pop)
        q = g.names["after_arr"]
        if kill == "acc":
            acc[g.start] = G.NEED_INF16
        elif kill == "pop":
            pop[q] = G.NEED_INF16
        elif kill == "obj":
            pop[g.pop_target[0]] = G.NEED_INF16
        else:
            acc[g.pop_target[2]] = G.NEED_INF16
        fake = type("B", (), {"g": g, "c_acc": acc, "c_pop": pop, "need": G.GrammarBudget.need})()
        cases = [(s[0], s[1], s[2], fake.need(s)) for s in ((g.start, 0, 0), (q, 1, 1), (q, 3, 0b101), (q, 3, 0b111))]
        assert any(c[3] == G.NEED_INF for c in cases)
        out.append((g, fake, cases))
    return out


def rule_cases():
    rows = []
    free = G.BUDGET_FREE
    for budget in (-5, -1, 0, 1, 2, 3, 50, free, free + 7, (1 << 31) - 1):
        for step in (-3, 0, 1, 2, 49, 50, 51, 8192, 1 << 40):
            r = max(-1, min(budget - max(step, 0), free))
            for need_after in (0, 1, r - 2, r - 1, 131, G.NEED_INF):
                for all_live, cap in ((0, 0), (1, 0), (1, r - 2), (1, r - 1), (1, G.NEED_INF)):
                    rows.append([budget, step, need_after, all_live, cap, r, int(r > 0 and need_after <= r - 2),
                                 int(bool(all_live) and r > 0 and cap <= r - 2)])
    return rows


BOK = OK + [S, S, 3]
# plan_grammar_mask's 15 arguments (tests/test_grammar_host_check.py), then need_states flag_states budget_rows


def plan(rc, chunks=0, **kw):
    names = ["B", "V", "ld", "dtype", "tab", "states", "classes", "byte_cap", "n_off", "n_bytes", "rows", "has_out",
             "has_step", "max_steps", "out_ld", "need_states", "flag_states", "budget_rows"]
    a = list(BOK)
    for k, v in kw.items():
        a[names.index(k)] = v
    return a + [rc, chunks]


PLANS = [
    plan(0, 501), plan(0, 501, dtype=1, ld=M + 8), plan(0, 1, V=33, ld=33), plan(0, 17, V=4099, ld=4104),
    plan(0, 501, has_out=1, has_step=1, max_steps=8192, out_ld=3), plan(0, 501, rows=64, budget_rows=64),
    plan(0, 501, states=100, need_states=100, flag_states=128), plan(0, 501, budget_rows=9),
    # every refusal of the plain plan comes first, unchanged
    plan(-1, V=0), plan(-1, ld=M - 1), plan(-2, V=(1 << 20) + 1, ld=1 << 21, n_off=1 << 22), plan(-3, dtype=2),
    plan(-4, tab=T + 8), plan(-4, tab=12), plan(-4, states=S + 1, need_states=S + 1, flag_states=S + 1), plan(-4, states=0),
    plan(-5, classes=C + 1), plan(-6, byte_cap=BYTE_CAP + 1), plan(-7, has_out=1), plan(-7, has_step=1),
    plan(-8, has_out=1, has_step=1, out_ld=2), plan(-9, n_off=M), plan(-9, n_bytes=1000), plan(-10, rows=2),
    # then the budget's own operands
    plan(-12, need_states=S - 1), plan(-12, flag_states=S - 1), plan(-12, flag_states=0), plan(-12, budget_rows=2),
    plan(-12, rows=64), plan(-12, need_states=-1),
]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_need_rule_plan_and_launcher_under_asan_ubsan(tmp_path):
    grammars, rules = need_cases(), rule_cases()
    nums = [len(grammars)]
    n_need = 0
    for g, bd, cases in grammars:
        nums += [g.n_states, *g.pop_target, *bd.c_acc, *bd.c_pop, len(cases)]
        for c in cases:
            nums += c
        n_need += len(cases)
    nums.append(len(rules))
    for r in rules:
        nums += r
    nums.append(len(PLANS))
    for p in PLANS:
        nums += p
    path = tmp_path / "cases.txt"
    path.write_text(" ".join(str(int(n)) for n in nums))
    exe = str(tmp_path / "grammar_budget_check")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(CSRC, "tests", "grammar_budget_check.cpp"), os.path.join(CSRC, "grammar_budget.hip"),
           "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    nm = shutil.which("nm")
    if nm:
        syms = subprocess.run([nm, exe], capture_output=True, text=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms   # the sanitizers really are linked in
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "0 failure(s)" in r.stdout and n_need > 2000 and len(rules) > 1000
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
