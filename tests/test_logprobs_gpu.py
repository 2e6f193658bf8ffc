"""csrc/logprobs.hip (the chosen token's log-probability and the top n_top alternatives, computed on
the device after K6) against the fp64 oracle (ops/oracle64.py) for bf16 and fp32 logits: ids exactly,
values within ``logprob_tol``; its graph form inside a captured step against the CPU reference; the
binding's refusals; and the engine's graph and eager paths. Each kernel case prints its worst
error / tolerance (``pytest -s``)."""
import math

import pytest
import torch

from theroundtaible_amd import ops
from theroundtaible_amd.engine import Engine, EngineConfig, SamplingParams, Turn
from theroundtaible_amd.ops import oracle64 as o64

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = ops.MAX_TOP_LOGPROBS
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
NAN_BITS = 0x7FC12345          # a quiet NaN with a payload: the records of rows that do not ask keep it


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def fresh_records(B, steps=1):
    """A LogProbs whose records hold NAN_BITS everywhere (ids as the same int32 pattern)."""
    lp = ops.LogProbs(B, DEV, steps)
    for t in (lp.tok_lp, lp.top_lp, lp.top_id):
        t.view(torch.int32).fill_(NAN_BITS)
    return lp


def check_case(what, logits, n_top, toks):
    """Run the two launches on ``logits`` (a CPU view, possibly of NaN-padded rows: the device copy
    keeps the layout) in the ``ids`` form and compare record row 0 with the oracle."""
    B, V = logits.shape
    ld = logits.stride(0)
    buf = torch.full((B, ld), float("nan"), dtype=logits.dtype, device=DEV)
    view = buf[:, :V]
    view.copy_(logits)
    before = bits(buf)
    lp = fresh_records(B)
    lp.n_top.copy_(n_top)
    ops.token_logprobs(view, lp, ids=toks.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), before), f"{what}: the logits (or the padding between rows) changed"
    if ld > V:
        assert bool(torch.isnan(buf[:, V:]).all()), f"{what}: the padding is no longer NaN"
    oracle = o64.token_logprobs(logits, n_top, toks)
    ratio = o64.assert_logprobs(lp.tok_lp[0], lp.top_id[0], lp.top_lp[0], oracle, n_top, what)
    print(f"RATIO logprobs {what} {ratio:.3f}")
    off = (n_top < 0).to(DEV)
    for t in (lp.tok_lp[0], lp.top_lp[0], lp.top_id[0]):
        assert bool((t.view(torch.int32)[off] == NAN_BITS).all()), f"{what}: a row with n_top = -1 was written"
    return lp, oracle


@DTYPES
@pytest.mark.parametrize("V", o64.LOGPROB_V, ids=lambda v: f"V{v}")
def test_kernel_matches_fp64_oracle(V, dtype):
    """B = 3 with n_top = (-1, 0, 20), every case kind, at the smallest V of every branch: fewer
    tokens than n_top (19), one partial chunk with NaN padding between the rows (1003, rows 1008
    apart), exactly one chunk (4096), a second chunk of one element (4097), 8 chunks with a partial
    last one (32064)."""
    for kind in o64.LOGPROB_KINDS:
        if kind == "big80" and dtype != torch.float32:
            continue
        logits, n_top, toks = o64.logprob_case(V, dtype, kind, ld=1008 if V == 1003 else None)
        assert n_top.tolist() == [-1, 0, 20]
        lp, (e_tok, e_id, e_lp, lse, _, _) = check_case(f"V={V} {dtype} {kind}", logits, n_top, toks)
        got_id = lp.top_id[0].cpu()
        if V < K:
            assert got_id[2, V:].tolist() == [-1] * (K - V) and bool((lp.top_lp[0, 2, V:] == -math.inf).all())
        if kind == "equal":
            n = min(K, V)
            assert got_id[2, :n].tolist() == list(range(n)), "ties go to the lower token id"
            assert torch.allclose(lp.top_lp[0, 2, :n].cpu().double(), torch.full((n,), -math.log(V), dtype=torch.float64),
                                  atol=float(o64.LOGPROB_SLACK * (1 + 1.625 + abs(float(lse[2])))), rtol=0)
        if kind == "banned300":
            assert bool((lp.tok_lp[0, 1:] == -math.inf).all()), "a banned token's logprob is -inf"
        if kind == "finite5" and V > 5:
            assert bool((lp.top_lp[0, 2, 5:min(K, V)] == -math.inf).all()) and bool((got_id[2, 5:min(K, V)] >= 0).all())


@DTYPES
def test_kernel_38_chunks(dtype):
    """V = 152064: 38 chunks, more than K6's 32."""
    logits, n_top, toks = o64.logprob_case(o64.LOGPROB_V_BIG, dtype, "random")
    check_case(f"V={o64.LOGPROB_V_BIG} {dtype} random", logits, n_top, toks)


@DTYPES
@pytest.mark.parametrize("kind", ["random", "levels8"])
def test_kernel_batch_32_mixed_n_top(kind, dtype):
    """B = 32, V = 4097, n_top mixed over -1, 0, 1, 5, 7, 19, 20; two chosen ids outside [0, V)
    give NaN (and read nothing)."""
    logits, n_top, toks = o64.logprob_case(4097, dtype, kind, B=32)
    lp, _ = check_case(f"B=32 V=4097 {dtype} {kind}", logits, n_top, toks)
    assert toks[-1] == 4097 and toks[-2] == -1 and n_top[-1] >= 0 and n_top[-2] >= 0
    assert bool(torch.isnan(lp.tok_lp[0, -2:]).all())


def test_binding_refusals():
    nat = ops.native()
    lp = ops.LogProbs(2, DEV, 4)
    args = lambda l: (l, lp.n_top, lp.ws, lp.tok_lp, lp.top_id, lp.top_lp)         # noqa: E731
    ids = torch.zeros(3, dtype=torch.int64, device=DEV)
    ok = torch.zeros(2, 64, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="bfloat16 or float32"):
        nat.token_logprobs(*args(torch.zeros(2, 64, dtype=torch.float16, device=DEV)), ids)
    with pytest.raises(RuntimeError, match="cover the batch"):
        nat.token_logprobs(*args(torch.zeros(3, 64, dtype=torch.float32, device=DEV)), ids)
    with pytest.raises(RuntimeError, match="logits must be"):
        nat.token_logprobs(*args(torch.zeros(2, 64, 2, device=DEV)[:, :, 0]), ids)
    out = torch.zeros(4, 2, dtype=torch.int64, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="go together"):
        nat.token_logprobs(*args(ok), None, out, None)
    with pytest.raises(RuntimeError, match="go together"):
        nat.token_logprobs(*args(ok), None, None, step)
    with pytest.raises(RuntimeError, match="cover the batch"):
        nat.token_logprobs(*args(ok), None, torch.zeros(4, 1, dtype=torch.int64, device=DEV), step)
    with pytest.raises(RuntimeError, match="cover the steps"):
        nat.token_logprobs(*args(ok), None, torch.zeros(5, 2, dtype=torch.int64, device=DEV), step)
    with pytest.raises(RuntimeError, match="rc=-4"):       # a record narrower than 20 columns
        nat.token_logprobs(ok, lp.n_top, lp.ws, lp.tok_lp, lp.top_id[:, :, :19].contiguous(),
                           lp.top_lp[:, :, :19].contiguous(), ids)
    with pytest.raises(RuntimeError, match="rc=-2"):       # V > 64 x 4096
        nat.token_logprobs(*args(torch.zeros(2, 64 * 4096 + 1, dtype=torch.bfloat16, device=DEV)), ids)
    with pytest.raises(RuntimeError, match="rc=-8"):       # workspace too small
        nat.token_logprobs(ok, lp.n_top, lp.ws[:100], lp.tok_lp, lp.top_id, lp.top_lp, ids)


# ---- the graph form inside a captured step -------------------------------------------------------

STEPS, CB, CV = 40, 3, 640


@DTYPES
def test_captured_step_records_every_replay(dtype):
    """Capture {logits <- seq[step], sample_advance (K6 + record + advance), token_logprobs(out,
    step)} once and replay it 40 times of 48 possible: record row s equals the CPU reference for
    the token out[s] on seq[s]; rows at and after ``step`` keep their bits; sampled ids are those of
    the same capture without the logprob launches."""
    g = torch.Generator().manual_seed(11)
    seq = (3.0 * torch.randn(STEPS, CB, CV, generator=g)).to(dtype)
    seq_d = seq.to(DEV)
    H, bs, maxb, ROWS = 64, 32, 4, 48
    embed = torch.randn(CV, H, generator=g).to(torch.bfloat16).to(DEV)
    bt = torch.arange(CB * maxb, dtype=torch.int32, device=DEV).reshape(CB, maxb)
    temp = torch.tensor([0.0, 0.8, 0.7], device=DEV)
    top_p = torch.tensor([1.0, 0.9, 1.0], device=DEV)
    top_k = torch.tensor([0, 0, 40], dtype=torch.int32, device=DEV)
    seeds = torch.tensor([5, 36, 67], dtype=torch.int64, device=DEV)
    n_top = torch.tensor([20, -1, 5], dtype=torch.int32)

    def run(with_lp):
        z = lambda dt: torch.zeros(CB, dtype=dt, device=DEV)                       # noqa: E731
        out = torch.zeros(ROWS, CB, dtype=torch.int64, device=DEV)
        step = torch.zeros(1, dtype=torch.int64, device=DEV)
        ids, pos, ctx, slots, offs = z(torch.int64), z(torch.int64), z(torch.int32), z(torch.int64), z(torch.int64)
        res = torch.zeros(CB, H, dtype=torch.bfloat16, device=DEV)
        logits = torch.zeros(CB, CV, dtype=dtype, device=DEV)
        nxt = z(torch.int64)
        ws = ops.sample_workspace(CB, DEV)
        lp = fresh_records(CB, ROWS)
        lp.n_top.copy_(n_top)

        def reset():
            for t in (out, step, ids, pos, slots):
                t.zero_()
            ctx.fill_(1)
            offs.fill_(1)
            for t in (lp.tok_lp, lp.top_lp, lp.top_id):
                t.view(torch.int32).fill_(NAN_BITS)

        def body():
            logits.copy_(torch.index_select(seq_d, 0, step.clamp(max=STEPS - 1))[0])
            ops.sample_advance(logits, temp, top_p, top_k, seeds, offs, ws, nxt, out, ids, pos, ctx, step, slots, res,
                               bt, embed, bs)
            if with_lp:
                ops.token_logprobs(logits, lp, out=out, step=step)

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
        for _ in range(STEPS):
            gr.replay()
        torch.cuda.synchronize()
        assert int(step.item()) == STEPS
        return out.cpu(), lp

    out, lp = run(True)
    plain, _ = run(False)
    assert torch.equal(out, plain), "ids with logprobs on differ from ids with them off"
    want = ops.LogProbs(CB, "cpu", 1)
    want.n_top.copy_(n_top)
    asking = n_top >= 0
    for s in range(STEPS):
        ops.token_logprobs(seq[s], want, ids=out[s])
        oracle = o64.token_logprobs(seq[s], n_top, out[s])
        assert torch.equal(lp.top_id[s].cpu()[asking], want.top_id[0][asking]), f"step {s}: ids vs the CPU reference"
        o64.assert_logprobs(lp.tok_lp[s], lp.top_id[s], lp.top_lp[s], oracle, n_top, f"captured step {s}")
        assert bool((lp.tok_lp[s, 1].view(torch.int32) == NAN_BITS).all()), "the row that does not ask was written"
    for t in (lp.tok_lp, lp.top_lp, lp.top_id):
        assert bool((t[STEPS:].view(torch.int32) == NAN_BITS).all()), "a record row at or after step was written"


# ---- engine ---------------------------------------------------------------------------------------

PROMPT = "Hallo tafel, wat is het plan voor vandaag?"


def eng(**kw):
    cfg = dict(model="tiny-llama-128", weights="random-full:3", device="cuda:0", num_blocks=512)
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


def greedy(**kw):
    return SamplingParams(temperature=0.0, max_new_tokens=16, ignore_eos=True, stop_on_consensus=False, **kw)


def close(a, b, what):
    """Two records of the same logits, from two launch forms (or two GEMM paths of the same model):
    bf16 logits feed both, so a differing logit moves by whole bf16 steps; compare loosely."""
    assert a[1] == b[1], f"{what}: top ids {a[1]} vs {b[1]}"
    for x, y in zip([a[0]] + a[2], [b[0]] + b[2]):
        assert (x == y) or abs(x - y) <= 0.05 * (1 + abs(y)), f"{what}: {x} vs {y}"


def test_engine_graph_path_records_and_cache_keys():
    """A logprobs=5 run's ids equal the plain run's bit for bit; the lp graph is cached beside the
    plain one under (key, "lp") and a following plain batch captures nothing new; records are
    consistent with a greedy choice."""
    e = eng(use_graphs=True)
    base = e.run_turns([Turn("K1", PROMPT, greedy())])[0]
    assert base.error is None and len(base.ids) == 16 and base.logprobs is None
    assert e.stats["graph_captures"] == 1 and len(e.graphs) == 1
    (key,) = e.graphs
    out = e.run_turns([Turn("K2", PROMPT, greedy(logprobs=5))])[0]
    assert out.error is None and out.ids == base.ids, "logprobs changed the sampled ids"
    assert set(e.graphs) == {key, (key, "lp")} and e.stats["graph_captures"] == 2
    assert len(out.logprobs) == 16
    for tok, (tok_lp, top_ids, top_lps) in zip(out.ids, out.logprobs):
        assert len(top_ids) == len(top_lps) == 5 and top_ids[0] == tok and tok_lp == top_lps[0]
        assert top_lps == sorted(top_lps, reverse=True)
        assert sum(math.exp(v) for v in top_lps) <= 1 + 1e-4
    again = e.run_turns([Turn("K3", PROMPT, greedy())])[0]
    assert again.ids == base.ids and again.logprobs is None
    assert e.stats["graph_captures"] == 2 and len(e.graphs) == 2, "a plain batch saw the lp graph"
    # sampled rows beside a row that does not ask: same ids as without logprobs
    sampled = dict(temperature=0.8, top_p=0.9, seed=5, max_new_tokens=16, ignore_eos=True, stop_on_consensus=False)
    plain = e.run_turns([Turn("S1", PROMPT, SamplingParams(**sampled)), Turn("S2", PROMPT + " Anders.", greedy())])
    for k in ("S1", "S2"):          # the RNG is keyed by (seed, sequence key, position): same keys, fresh sequences
        e.release(k)
    both = e.run_turns([Turn("S1", PROMPT, SamplingParams(**sampled, logprobs=20)),
                        Turn("S2", PROMPT + " Anders.", greedy())])
    assert [o.ids for o in both] == [o.ids for o in plain] and both[1].logprobs is None
    assert all(r[0] <= r[2][0] <= 0 and len(r[1]) == 20 for r in both[0].logprobs)
    # the eager path gives the same records wherever its ids agree
    eager = eng(use_graphs=False).run_turns([Turn("K2", PROMPT, greedy(logprobs=5))])[0]
    assert len(eager.logprobs) == 16
    n = next((i for i, (a, b) in enumerate(zip(eager.ids, out.ids)) if a != b), 16)
    assert n >= 1
    for i in range(n):
        close(eager.logprobs[i], out.logprobs[i], f"eager vs graph, token {i}")


def test_engine_banned_token_is_minus_infinity_where_listed():
    """logit_bias -100 on the plain run's tokens with logprobs=20: the (key, "proc", "lp") graph; the
    logprobs are those of the PROCESSED logits, so no banned token is the chosen one or outranks it,
    and a banned token's entry, where it is listed at all, is -inf."""
    e = eng(use_graphs=True)
    base = e.run_turns([Turn("K1", PROMPT, greedy())])[0]
    (key,) = e.graphs
    bans = {a: -100.0 for a in set(base.ids)}
    out = e.run_turns([Turn("K2", PROMPT, greedy(logit_bias=bans, logprobs=20))])[0]
    assert out.error is None and not set(out.ids) & set(base.ids)
    assert set(e.graphs) == {key, (key, "proc", "lp")}
    same = e.run_turns([Turn("K3", PROMPT, greedy(logit_bias=bans))])[0]
    assert same.ids == out.ids and (key, "proc") in e.graphs
    for tok, (tok_lp, top_ids, top_lps) in zip(out.ids, out.logprobs):
        assert top_ids[0] == tok
        for i, v in zip(top_ids, top_lps):
            if i in bans:
                assert v == -math.inf, (i, v, tok_lp)
