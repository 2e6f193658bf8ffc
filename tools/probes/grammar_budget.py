"""Probe: what the budgeted grammar mask (csrc/grammar_budget.hip) costs beside the plain one
(csrc/grammar_mask.hip, unchanged from the commit that introduced it), in one process on one box.

B = 3 rows, V = 128256, bf16 logits; token table: the bundled byte-level BPE plus the printable fallback
pieces of the ids above it; all three rows carry the same grammar at the same state (the method of
profiles/r11/grammar/README.md: 20 calls of the op captured in one graph, the graph replayed 30 times
between two device events, median of 5 windows after warm-up; µs per call, kernel boundary included).
The configurations alternate, ROUNDS times over, so that a drift of the box shows in every column:

* ``plain``     grammar_mask, json_object at its start state (the earlier record: 21-29 µs)
* ``a``         the budgeted launch, same state, rows without grammar_finish (zero need arrays, free budget)
* ``b``         the budgeted launch, same state, grammar_finish with a budget that binds (r = need + 3)
* ``c``         the budgeted launch in the free phase of the knights' consensus ``tail`` grammar with a
                budget far above need_cap: the shortcut (no table staged, no token walked)
* ``c-walked``  the same state with r - 2 one below need_cap: the table is read and every token walked
* ``... +step`` the captured-step form of ``plain``, ``a`` and ``c``: the state is slot 0 advanced over one
                recorded token (a space, which leaves both states where they are) at a fixed ``*step = 1``,
                r = budget - 1; the step counter does not move, so every call does the same work

Every masked row is compared with ops/reference.py on the host before it is timed.

    python tools/probes/grammar_budget.py --out table.md
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from theroundtaible_amd import ops  # noqa: E402
from theroundtaible_amd.consensus import consensus_grammar  # noqa: E402
from theroundtaible_amd.engine import grammar as G  # noqa: E402
from theroundtaible_amd.engine.tokenizer import EngineTokenizer  # noqa: E402
from theroundtaible_amd.ops import reference as ref  # noqa: E402

DEV = "cuda"
B, V = 3, 128256
REP, REPLAYS, WARM, WINDOWS, ROUNDS = 20, 30, 5, 5, 3


def capture(body):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REP):
            body()
    for _ in range(WARM):
        g.replay()
    torch.cuda.synchronize()
    return g


def time_graph(g) -> float:
    """µs per call: the median of WINDOWS windows of REPLAYS replays."""
    times = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPLAYS):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / (REPLAYS * REP))
    return statistics.median(times)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tok = EngineTokenizer(V)
    table = G.token_table(tok, V)
    jb = G.bind({"type": "json_object"}, tok, V)
    tb = G.bind(consensus_grammar(), tok, V)
    jst, tst = jb.g.start_state, tb.g.start_state
    cap = tb.budget().need_cap
    assert tb.all_live()[tst[0]] == 1
    base = (3.0 * torch.randn(B, V, generator=torch.Generator().manual_seed(1))).to(torch.bfloat16)
    configs = [("plain", jb, jst, False, None, False), ("a", jb, jst, True, None, False),
               ("b", jb, jst, True, jb.budget().need(jst) + 3, False), ("c", tb, tst, True, cap + 500, False),
               ("c-walked", tb, tst, True, cap + 1, False), ("plain +step", jb, jst, False, None, True),
               ("a +step", jb, jst, True, None, True), ("c +step", tb, tst, True, cap + 500, True)]
    space = table.pieces.index(b" ")
    assert jb.advance(jst, space) == jst and tb.advance(tst, space) == tst
    graphs, allowed, keep = {}, {}, []
    for name, bound, st, budgeted, left, stepped in configs:
        if budgeted:
            gm_d = ops.GrammarBudgetMask(B, DEV, table).fill([(bound, st, left)] * B)
            gm_h = ops.GrammarBudgetMask(B, "cpu", table).fill([(bound, st, left)] * B)
            op, rop = ops.apply_grammar_mask_budget, ref.apply_grammar_mask_budget
        else:
            gm_d = ops.GrammarMask(B, DEV, table).fill([(bound, st)] * B)
            gm_h = ops.GrammarMask(B, "cpu", table).fill([(bound, st)] * B)
            op, rop = ops.apply_grammar_mask, ref.apply_grammar_mask
        logits = base.clone().to(DEV)
        rec = (torch.full((2, B), space, dtype=torch.int64), torch.ones(1, dtype=torch.int64)) if stepped else (None, None)
        rec_d = tuple(None if t is None else t.to(DEV) for t in rec)
        want = rop(base.clone(), gm_h, *rec)
        got = op(logits, gm_d, *rec_d).cpu()
        assert not stepped or gm_d.states(1) == gm_h.states(1) == [st] * B
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{name}: the kernel and the reference differ"
        allowed[name] = int(torch.isfinite(want[0].float()).sum())
        graphs[name] = capture(lambda op=op, logits=logits, gm_d=gm_d, rec_d=rec_d: op(logits, gm_d, *rec_d))
        keep.append((logits, gm_d, rec_d))
    rows = {name: [] for name, *_ in configs}
    for _ in range(ROUNDS):
        for name, *_ in configs:
            rows[name].append(time_graph(graphs[name]))
    lines = ["| configuration | allowed | µs per launch, round by round | median |", "|---|---|---|---|"]
    for name, *_ in configs:
        lines.append(f"| {name} | {allowed[name]} | {', '.join(f'{t:.1f}' for t in rows[name])} | "
                     f"{statistics.median(rows[name]):.1f} |")
    text = "\n".join(lines) + f"\n\nneed_cap of the consensus grammar: {cap}; its table: {tb.g.n_states} x {tb.g.n_classes}\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
