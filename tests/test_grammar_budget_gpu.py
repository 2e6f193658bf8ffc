"""csrc/grammar_budget.hip on the device: the budgeted mask against ops/reference.py bit for bit (every output
is an integer decision: no tolerance) over states, budgets and the free-phase shortcut; the captured step's
state and budget hand-over against the CPU walker; the engine's graph and eager paths with
``grammar_finish`` and a ``tail`` grammar (no whitespace ban, temperature 1: the budget is what ends the
reply); and which graph a batch captures."""
import json
import random

import pytest
import torch

from test_grammar_gpu import FINITE, JSON_PREFIXES, NESTING, PROMPT, bits, eng, valid
from theroundtaible_amd import ops
from theroundtaible_amd.engine import SamplingParams, Turn
from theroundtaible_amd.engine import grammar as G
from theroundtaible_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = G.GRAMMAR_MAX_DEPTH
BYTE_CAP = G.GRAMMAR_TOKEN_BYTE_CAP
JSON = G.compile_grammar({"type": "json_object"})
TAIL = G.compile_grammar({"type": "tail", "open": "~~", "body": {"type": "regex", "pattern": "(tr|fa)+,?"}, "close": "]"})
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
LARGE = 5000


def budget_table(V: int) -> G.TokenTable:
    """Zero-byte specials (ids 0, 1, 2 and the last id; 1 and the last are stop ids), single bytes through
    which every state of both grammars can be left (V = 33: just those; else all 256), tokens that cross
    the tail grammar's seam — ``~q`` holds the end of the opener and then a byte no body starts with, so
    it clears the all-live flag of the free state after one ``~`` and of no other — and, for the large
    table, nesting tokens and random strings up to the byte cap + 1 (none holds ``~``)."""
    rng = random.Random(V)
    pieces = [b"", b"", b""]
    if V < 300:
        pieces += [bytes([b]) for b in b'{}[]":,1 \\uetrfalsn-.~\x85\xa9'] + [b'{"', b"]}", b"~~t", b"~q", b"tr,"]
    else:
        pieces += [bytes([b]) for b in range(256)] + NESTING + [b"~~t", b"~q", b"tr,", b"~~tr]", b"x~"]
    alphabets = [b'{}[]":,\\ 0123456789.-+eEtruefalsn ab\xc3\xa9', b"abcdefgh ", b"0123456789"]
    k = 0
    while len(pieces) < V:
        n = (2, 3, 17, 64, BYTE_CAP, BYTE_CAP + 1)[k % 6]
        pieces.append(bytes(rng.choice(alphabets[(k // 6) % 3]) for _ in range(n)))
        k += 1
    pieces = pieces[:V - 1] + [b""]
    return G.TokenTable(pieces, [1, V - 1], name=f"budget{V}")


JSON_STATES = [n for n in ("start", "in string", "mid UTF-8", "number in array", "after a value at depth 1", "depth = cap",
                           "arrays to the cap", "done")]
TAIL_PREFIXES = [("free", b"some text"), ("free after one ~", b"x~"), ("body", b"~~t"), ("accepting", b"~~trfa,]"),
                 ("body after a pair", b"q~~tr")]


@DTYPES
@pytest.mark.parametrize("V,pad", [(4099, 0), (4099, 5), (33, 0), (33, 7)], ids=["V4099", "V4099_ld4104", "V33", "V33_ld40"])
def test_budgeted_mask_matches_the_reference_bit_for_bit(V, pad, dtype):
    table = budget_table(V)
    jb, tb = G.BoundGrammar(JSON, table), G.BoundGrammar(TAIL, table)
    jbd, tbd = jb.budget(), tb.budget()
    s0, s1 = TAIL.walk(TAIL.start_state, b"")[0], TAIL.walk(TAIL.start_state, b"~")[0]
    assert tbd.need_cap == 5 == tbd.need(TAIL.start_state) and [q for q, f in enumerate(tbd.all_live) if f] == [s0]
    assert s1 != s0 and sum(jbd.all_live) == 0
    gm_d, gm_h = ops.GrammarBudgetMask(3, DEV, table), ops.GrammarBudgetMask(3, "cpu", table)
    g = torch.Generator().manual_seed(V)
    prefixes = dict(JSON_PREFIXES)
    states = [(n, JSON.walk(JSON.start_state, prefixes[n])) for n in JSON_STATES] + [("FIN", G.FIN), ("DEAD", G.DEAD)]
    assert states[5][1][1] == CAP and states[6][1][1] == CAP and all(st[0] >= 0 for _, st in states[:-2])
    tstates = [(n, TAIL.walk(TAIL.start_state, p)) for n, p in TAIL_PREFIXES] + [("FIN", G.FIN)]
    seen_skip = set()
    for k, (name, st) in enumerate(states):
        tname, tst = tstates[k % len(tstates)]
        need, tneed = jbd.need(st), tbd.need(tst)
        # r: the budget exhausted, its last token, the need itself and one / two above it (two above is the
        # first budget every token of the shortest way fits, and for the flagged free state the first one
        # at which no token is walked: need_cap <= r - 2), and one that binds nothing
        for r, tr in zip((-1, 0, 1, need, need + 1, need + 2, LARGE, None),
                         (tneed + 2, LARGE, tneed + 1, -1, 0, 1, tneed, None)):
            if r is None or r == -1:    # operands once per state pair and kind of row; the other budgets only
                rows = [(jb, st, r), (tb, tst, tr), None]       # rewrite `budget`, as the eager path does per step
                gm_d.fill(rows)
                gm_h.fill(rows)
            else:
                gm_d.set_budgets([r, tr, None])
                gm_h.set_budgets([r, tr, None])
            if tst[0] == s0 and tr is not None:
                seen_skip.add(tr > 0 and tbd.need_cap <= tr - 2)
            logits = (3.0 * torch.randn(3, V, generator=g)).to(dtype)
            logits[0, 5] = float("-inf")                        # an element that is -inf already
            buf = torch.full((3, V + pad), float("nan"), dtype=dtype, device=DEV)
            view = buf[:, :V]
            view.copy_(logits)
            assert ops.apply_grammar_mask_budget(view, gm_d).data_ptr() == buf.data_ptr()
            want = ref.apply_grammar_mask_budget(logits.clone(), gm_h)
            got = view.cpu()
            where = f"{name} r={r} / {tname} r={tr}"
            assert torch.equal(bits(got), bits(want)), f"{where}: the kernel and the reference differ"
            masked = torch.isinf(want.float()) & (want.float() < 0)
            assert torch.equal(bits(got)[~masked], bits(logits)[~masked]), f"{where}: an allowed element changed"
            assert torch.equal(bits(got[2]), bits(logits[2])), f"{where}: the row without a grammar changed"
            # (need <= r - 1 holds at every step of a real reply; a state paired with a smaller r cannot occur
            # there and may lose every element)
            for b, (n, left) in enumerate(((need, r), (tneed, tr))):
                if left is None or left <= 0 or left >= n + 1:
                    assert bool((~masked[b]).any()), f"{where}: row {b} without a finite element"
            if pad:
                assert bool(torch.isnan(buf[:, V:]).all()), f"{where}: wrote past column V"
            free = G.BUDGET_FREE
            for i in range(V if pad == 0 and V < 300 else 0):     # the reference against the scalar rule
                assert bool(masked[0, i]) == (not jb.token_allowed_budget(st, i, free if r is None else r) or i == 5), (where, i)
                assert bool(masked[1, i]) == (not tb.token_allowed_budget(tst, i, free if tr is None else tr)), (where, i)
            assert gm_d.states(0) == gm_h.states(0)             # step=None: the state is only read
            if r is None:       # nothing binds: the plain launch's result
                plain = ops.apply_grammar_mask(logits.clone().to(DEV), ops.GrammarMask(3, DEV, table).fill([(jb, st), (tb, tst), None]))
                assert torch.equal(bits(plain), bits(got)), f"{where}: differs from grammar_mask"
    assert seen_skip == {True, False}       # the flagged free state on both sides of need_cap


def test_launcher_refusals():
    table = budget_table(33)
    gm = ops.GrammarBudgetMask(2, DEV, table)
    with pytest.raises(ValueError, match="token table"):
        ops.apply_grammar_mask_budget(torch.zeros(2, 34, device=DEV), gm)
    with pytest.raises(RuntimeError):
        ops.apply_grammar_mask_budget(torch.zeros(2, 33, dtype=torch.float16, device=DEV), gm)
    with pytest.raises(RuntimeError):
        ops.apply_grammar_mask_budget(torch.zeros(3, 33, device=DEV), gm)          # operands cover 2 rows
    args = [gm.meta, gm.cls, gm.tab, gm.accept, gm.stops, gm.state, gm.tok_off, gm.tok_bytes]
    for budget, need, flags in ((gm.budget[:1], gm.need, gm.all_live), (gm.budget, gm.need[:, :, :100].contiguous(), gm.all_live),
                                (gm.budget, gm.need, gm.all_live[:, :100].contiguous()), (gm.budget, gm.need[:1], gm.all_live)):
        with pytest.raises(RuntimeError):
            ops.native().grammar_mask_budget(torch.zeros(2, 33, device=DEV), *args, budget, need, flags)


# ---- the captured step --------------------------------------------------------------------------------------

STEPS, CB, CV = 40, 3, 4099
BUDGETS = [30, 24]


@DTYPES
def test_captured_step_hands_state_and_budget_over(dtype):
    """Capture {logits <- seq[step], budgeted mask(out, step), sample_advance} once and replay it 40 times
    with no host input. Row 0: a tail grammar with 30 tokens, row 1: json_object with 24, row 2: no grammar.
    After replay s the slot s & 1 holds the CPU walker's state after out[0:s]; every recorded id is one the
    walker allows with budget - s tokens left; each reply ends with a stop id inside its budget, only stop
    ids follow, and its text is accepted; the plain row's logits pass through with their bits."""
    table = budget_table(CV)
    bounds = [G.BoundGrammar(TAIL, table), G.BoundGrammar(JSON, table), None]
    g = torch.Generator().manual_seed(23)
    seq = (3.0 * torch.randn(STEPS, CB, CV, generator=g)).to(dtype)
    seq_d = seq.to(DEV)
    H, bs, maxb, ROWS = 64, 32, 4, 48
    embed = torch.randn(CV, H, generator=g).to(torch.bfloat16).to(DEV)
    bt = torch.arange(CB * maxb, dtype=torch.int32, device=DEV).reshape(CB, maxb)
    temp = torch.tensor([1.0, 1.0, 0.7], device=DEV)
    top_p = torch.tensor([1.0, 1.0, 1.0], device=DEV)
    top_k = torch.tensor([0, 0, 40], dtype=torch.int32, device=DEV)
    seeds = torch.tensor([5, 36, 67], dtype=torch.int64, device=DEV)
    start = [(b, b.g.start_state, n) for b, n in zip(bounds[:2], BUDGETS)] + [None]

    def run(check_states):
        z = lambda dt: torch.zeros(CB, dtype=dt, device=DEV)                       # noqa: E731
        out = torch.zeros(ROWS, CB, dtype=torch.int64, device=DEV)
        step = torch.zeros(1, dtype=torch.int64, device=DEV)
        ids, pos, ctx, slots, offs = z(torch.int64), z(torch.int64), z(torch.int32), z(torch.int64), z(torch.int64)
        res = torch.zeros(CB, H, dtype=torch.bfloat16, device=DEV)
        logits = torch.zeros(CB, CV, dtype=dtype, device=DEV)
        snap = torch.zeros(CV, dtype=dtype, device=DEV)
        nxt = z(torch.int64)
        ws = ops.sample_workspace(CB, DEV)
        gm = ops.GrammarBudgetMask(CB, DEV, table)

        def reset():
            for t in (out, step, ids, pos, slots):
                t.zero_()
            ctx.fill_(1)
            offs.fill_(1)
            gm.fill(start)

        def body():
            logits.copy_(torch.index_select(seq_d, 0, step.clamp(max=STEPS - 1))[0])
            ops.apply_grammar_mask_budget(logits, gm, out, step)
            snap.copy_(logits[2])
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
                assert torch.equal(bits(snap), bits(seq[k, 2])), f"replay {k}: the plain row's logits changed"
                for b, bound in enumerate(bounds):
                    if bound is None:
                        continue
                    assert slot[b] == states[b], f"replay {k} row {b}: slot {k & 1} holds {slot[b]}, the walker {states[b]}"
                    assert bound.token_allowed_budget(states[b], rec[b], BUDGETS[b] - k), \
                        f"replay {k} row {b}: id {rec[b]} at {states[b]} with {BUDGETS[b] - k} left"
                    states[b] = bound.advance(states[b], rec[b])
        torch.cuda.synchronize()
        assert int(step.item()) == STEPS
        return out[:STEPS].cpu()

    out = run(True)
    assert torch.equal(out, run(False)), "two captures replayed different ids"
    stops = set(table.stop_ids)
    for b, bound in enumerate(bounds[:2]):
        col = out[:, b].tolist()
        first = min(k for k, t in enumerate(col) if t in stops)
        assert first < BUDGETS[b] and set(col[first:]) <= stops, f"row {b}: no stop id inside the budget"
        assert bound.g.accepts(b"".join(table.pieces[t] for t in col[:first]))
    plain = ops.sample(seq_d[0], temp, top_p, top_k, seeds, torch.ones(CB, dtype=torch.int64, device=DEV)).cpu()
    assert int(out[0, 2]) == int(plain[2])


# ---- engine ---------------------------------------------------------------------------------------------

TAIL_SPEC = {"type": "tail", "open": "```json\n", "body": {"type": "json_schema", "schema": FINITE}, "close": "\n```"}


@pytest.fixture(scope="module")
def engines():
    return eng(use_graphs=True), eng(use_graphs=False)


def params(seed, n, **kw):
    return SamplingParams(temperature=1.0, top_p=1.0, seed=seed, max_new_tokens=n, stop_on_consensus=False, **kw)


def both(engines, turns):
    ge, ee = engines
    graph, eager = ge.run_turns(turns), ee.run_turns(turns)
    for e in engines:
        for t in turns:
            e.release(t.seq_key)
    for a, b in zip(graph, eager):
        assert a.error is None and b.error is None, (a.error, b.error)
        assert a.ids == b.ids, "the graph path and the eager path sampled different ids"
    return graph


def test_engine_json_object_finishes_inside_24_and_48_tokens(engines):
    ge = engines[0]
    eos = ge.tokenizer.eos_id
    turns = [Turn(f"J{n}-{seed}", PROMPT, params(seed, n, grammar={"type": "json_object"}, grammar_finish=True))
             for n in (24, 48) for seed in (1, 2)]
    for t, o in zip(turns, both(engines, turns)):
        assert len(o.ids) <= t.params.max_new_tokens and o.ids[-1] == eos and eos not in o.ids[:-1]
        assert isinstance(json.loads(o.text), dict), o.text
    assert any("grb" in k for k in ge.graphs if isinstance(k[-1], str)) and not any("gr" in k for k in ge.graphs if isinstance(k[-1], str))
    with pytest.raises(ValueError, match="the minimum is 3"):
        ge.run_turns([Turn("short", PROMPT, params(1, 2, grammar={"type": "json_object"}, grammar_finish=True))])


def test_engine_tail_turn_is_free_text_and_a_fenced_block(engines):
    ge = engines[0]
    eos = ge.tokenizer.eos_id
    turns = [Turn("T1", PROMPT, params(3, 96, grammar=TAIL_SPEC, grammar_finish=True)),
             Turn("T2", PROMPT + " Kort.", params(4, 96, grammar=TAIL_SPEC, grammar_finish=True)),
             Turn("P", PROMPT, params(5, 96, ignore_eos=True))]
    outs = both(engines, turns)
    for o in outs[:2]:
        assert len(o.ids) <= 96 and o.ids[-1] == eos and eos not in o.ids[:-1]
        at = o.text.index("```json\n")
        assert o.text.endswith("\n```") and valid(json.loads(o.text[at + 8:-4])), o.text
    assert len(outs[2].ids) == 96


def test_graph_caching_by_batch(engines):
    """A batch of plain grammars still captures the "gr" graph, a batch without grammars the plain one; only a
    batch with a grammar_finish or tail row captures "grb", and then for all its grammar rows."""
    ge = eng(use_graphs=True)
    tags = lambda: sorted(k[-1] for k in ge.graphs if isinstance(k[-1], str))      # noqa: E731
    bias = {i: -100.0 for i, p in enumerate(ge.token_table().pieces) if p and not p.strip(b" \t\n\r")}
    plain = params(1, 12, ignore_eos=True)
    ge.run_turns([Turn("Q", PROMPT, plain)])
    assert tags() == [] and ge.stats["graph_captures"] == 1
    ge.run_turns([Turn("G", PROMPT, params(2, 16, grammar={"type": "json_object"}, logit_bias=bias))])
    assert tags() == ["gr"] and ge.stats["graph_captures"] == 2
    ge.run_turns([Turn("F", PROMPT, params(3, 16, grammar={"type": "json_object"}, grammar_finish=True))])
    assert tags() == ["gr", "grb"] and ge.stats["graph_captures"] == 3
    ge.run_turns([Turn("Q2", PROMPT, plain), Turn("G2", PROMPT, params(2, 16, grammar={"type": "json_object"}, logit_bias=bias))])
    ge.run_turns([Turn("Q3", PROMPT, plain)])
    assert tags() == ["gr", "gr", "grb"] and ge.stats["graph_captures"] == 4      # B = 2: its own "gr" graph; Q3 replays Q's
