"""csrc/logit_proc.hip (logit_bias, repetition, frequency and presence penalties on the device) against
the fp64 oracle (ops/oracle64.py) within one ulp of the storage dtype, its device-side history inside
a captured step bit for bit against the CPU reference loop, and the engine's graph path with bans.
Each kernel case prints its worst error / tolerance (``pytest -s``)."""
import pytest
import torch

from theroundtaible_amd import ops
from theroundtaible_amd.engine import Engine, EngineConfig, SamplingParams, Turn
from theroundtaible_amd.ops import oracle64 as o64
from theroundtaible_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("hist", "hist_len", "reply_from", "rp", "last_n", "pp", "fp", "bias_tok", "bias_val", "bias_n")


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def to_dev(proc):
    d = ops.LogitProc(proc.hist.shape[0], DEV, hist_cap=proc.hist.shape[1], bias_cap=proc.bias_tok.shape[1])
    for f in FIELDS:
        getattr(d, f).copy_(getattr(proc, f))
    return d


def check_kernel(what, logits, proc, out, step, ld_pad=0):
    """Run the kernel on a copy of ``logits`` (rows ``ld_pad`` elements apart from contiguous) and
    compare with the oracle: named elements within tolerance, every other element bit-equal."""
    B, V = logits.shape
    dt = logits.dtype
    buf = torch.full((B, V + ld_pad), float("nan"), dtype=dt, device=DEV)
    view = buf[:, :V]
    view.copy_(logits)
    res = ops.apply_logit_processors(view, to_dev(proc), out.to(DEV) if out is not None else None,
                                     step.to(DEV) if step is not None else None)
    assert res.data_ptr() == buf.data_ptr()
    got = view.cpu()
    e, mag, named = o64.apply_logit_processors(logits, proc, out, step)
    ratio = o64.assert_within(got, e, o64.logit_proc_tol(e, mag, dt), what, dtype=dt)
    print(f"RATIO logit_proc {what} {ratio:.3f} named={int(named.sum())}")
    assert torch.equal(bits(got)[~named], bits(logits)[~named]), f"{what}: an element no token names changed"
    assert torch.equal(bits(got[0]), bits(logits[0])), f"{what}: the neutral row changed"
    if ld_pad:
        assert bool(torch.isnan(buf[:, V:]).all()), f"{what}: wrote between the rows"
    return named


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V,pad", [(32064, 0), (1003, 5)], ids=["V32064", "V1003_ld1008"])
def test_kernel_matches_fp64_oracle(V, pad, dtype):
    """B = 3 (neutral / penalties / penalties + 300 biases); histories of 0, 1, 2048 and 3000 host
    tokens with the device record at step 0, 1 and 2500; tokens t, t + 4096, t + 8192 share a home
    slot; negative, zero, positive and -inf logits at the penalised tokens; ids outside [0, V)."""
    for n_hist in o64.LOGIT_PROC_HIST:
        for step in o64.LOGIT_PROC_STEPS:
            logits, proc, out, st = o64.logit_proc_case(V, dtype, n_hist, step)
            named = check_kernel(f"V={V} {dtype} hist={n_hist} step={step}", logits, proc, out, st, ld_pad=pad)
            assert bool(named[2].any()) and not bool(named[0].any())
            assert bool(torch.isinf(logits[1:][named[1:]]).any()), "no -inf logit at a named token"


def test_kernel_host_history_only():
    """``step=None`` (the eager path and the first token after prefill): ``out`` is not read."""
    logits, proc, out, _ = o64.logit_proc_case(32064, torch.bfloat16, 2048, 0)
    check_kernel("host only", logits, proc, None, None)


def test_kernel_full_table():
    """2048 distinct history tokens and 300 more distinct bias tokens: the 4096-slot table at its
    highest load (2348 keys), every token a multiple of 8 so that home slots collide in runs."""
    V, B = 32064, 3
    g = torch.Generator().manual_seed(77)
    toks = (torch.randperm(V // 8, generator=g)[:2348] * 8).to(torch.int32)
    logits = (4.0 * torch.randn(B, V, generator=g)).to(torch.bfloat16)
    proc = ops.LogitProc(B, "cpu", hist_cap=2048)
    for b in (1, 2):
        proc.hist[b] = toks[:2048]
    proc.hist_len.copy_(torch.tensor([0, 2048, 2048], dtype=torch.int32))
    proc.rp.copy_(torch.tensor([1.0, 1.5, 1.1]))
    proc.last_n.fill_(-1)
    proc.fp.copy_(torch.tensor([0.0, 0.5, 0.25]))
    proc.bias_tok[2] = toks[2048:]
    proc.bias_val[2] = 10.0 * torch.randn(300, generator=g)
    proc.bias_n[2] = 300
    named = check_kernel("full table", logits, proc, None, None)
    assert int(named[1].sum()) == 2048 and int(named[2].sum()) == 2348


def test_binding_refusals():
    proc = ops.LogitProc(2, DEV)
    with pytest.raises(RuntimeError, match="bfloat16 or float32"):
        ops.apply_logit_processors(torch.zeros(2, 64, dtype=torch.float16, device=DEV), proc)
    with pytest.raises(RuntimeError, match="cover the batch"):
        ops.apply_logit_processors(torch.zeros(3, 64, dtype=torch.float32, device=DEV), proc)
    with pytest.raises(RuntimeError, match="logits must be"):
        ops.apply_logit_processors(torch.zeros(2, 64, 2, device=DEV)[:, :, 0], proc)


# ---- the device-side history inside a captured step ----------------------------------------------

STEPS, CB, CV = 40, 3, 640


def exact_case(dtype):
    """-> (seq [40, B, V], proc, ids [40, B] of the CPU reference loop).

    Logits are multiples of 0.25 in [-8, 8] and the parameters (rp 2, fp 0.5, pp 0.25, biases
    +-1.5) keep every fp32 operation exact. 24 hot tokens per row take the 24 levels 2.0 ... 7.75 in
    a fresh order every step and the rest lie in [-8, 0], so the greedy choice is decided by the
    penalties the tokens generated so far have drawn. A step's draw is repeated until the
    processed rows each have a unique maximum (the reference loop runs alongside)."""
    g = torch.Generator().manual_seed(2024)
    proc = ops.LogitProc(CB, "cpu", hist_cap=64)
    hot = torch.stack([torch.randperm(CV, generator=g)[:24] for _ in range(CB)])
    proc.hist[:, :5] = hot[:, :5].to(torch.int32)           # the host part names hot tokens too
    proc.hist_len.fill_(5)
    proc.reply_from.copy_(torch.tensor([0, 3, 5], dtype=torch.int32))
    proc.rp.copy_(torch.tensor([1.0, 2.0, 2.0]))
    proc.last_n.copy_(torch.tensor([64, 8, -1], dtype=torch.int32))
    proc.fp.copy_(torch.tensor([0.0, 0.5, 0.5]))
    proc.pp.copy_(torch.tensor([0.0, 0.25, 0.25]))
    proc.bias_tok[2, :24] = hot[2].to(torch.int32)
    proc.bias_val[2, :24] = torch.tensor([1.5, -1.5]).repeat(12)
    proc.bias_n[2] = 24
    levels = 2.0 + 0.25 * torch.arange(24)
    seq = torch.empty(STEPS, CB, CV, dtype=dtype)
    out = torch.zeros(64, CB, dtype=torch.int64)
    step = torch.zeros(1, dtype=torch.int64)
    for k in range(STEPS):
        for _ in range(200):
            lg = torch.randint(-32, 1, (CB, CV), generator=g).float() * 0.25
            for b in range(CB):
                lg[b, hot[b]] = levels[torch.randperm(24, generator=g)]
            lg = lg.to(dtype)
            done = ref.apply_logit_processors(lg.clone(), proc, out, step).float()
            top = done.topk(2, dim=-1).values
            if bool((top[:, 0] > top[:, 1]).all()):
                break
        else:
            raise AssertionError(f"step {k}: no draw with a unique maximum per row")
        seq[k] = lg
        out[k] = done.argmax(-1)
        step += 1
    return seq, proc, out[:STEPS]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_captured_step_reads_device_history(dtype):
    """Capture {logits <- seq[step], processors, greedy K6, decode_advance} once, replay it 40
    times with no host input: the recorded ids equal the CPU reference loop token for token."""
    seq, proc, want = exact_case(dtype)
    plain = seq.float().argmax(-1)
    assert torch.equal(plain[:, 0], want[:, 0]), "the neutral row"
    assert int((plain[:, 1:] != want[:, 1:]).sum()) >= 20, "the penalties hardly ever change the greedy choice"
    seq_d, proc_d = seq.to(DEV), to_dev(proc)
    zeros = lambda dt: torch.zeros(CB, dtype=dt, device=DEV)                           # noqa: E731
    out = torch.zeros(64, CB, dtype=torch.int64, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    ids, pos, ctx = zeros(torch.int64), zeros(torch.int64), torch.ones(CB, dtype=torch.int32, device=DEV)
    temp, top_p, top_k, seeds = zeros(torch.float32), torch.ones(CB, device=DEV), zeros(torch.int32), zeros(torch.int64)
    logits = torch.zeros(CB, CV, dtype=dtype, device=DEV)
    nxt = zeros(torch.int64)
    ws = ops.sample_workspace(CB, DEV)

    def body():
        logits.copy_(torch.index_select(seq_d, 0, step)[0])
        ops.apply_logit_processors(logits, proc_d, out, step)
        ops.sample(logits, temp, top_p, top_k, seeds, pos, out=nxt, ws=ws)
        ops.decode_advance(out, ids, pos, ctx, step, nxt)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()                                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    for t in (out, step, ids, pos):
        t.zero_()
    ctx.fill_(1)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    for t in (out, step, ids, pos):
        t.zero_()
    ctx.fill_(1)
    for _ in range(STEPS):
        g.replay()
    torch.cuda.synchronize()
    assert int(step.item()) == STEPS
    assert out[:STEPS].cpu().tolist() == want.tolist()


# ---- engine ---------------------------------------------------------------------------------------

def eng(**kw):
    cfg = dict(model="tiny-llama-128", weights="random-full:3", device="cuda:0", num_blocks=512)
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


def greedy(**kw):
    return SamplingParams(temperature=0.0, max_new_tokens=16, ignore_eos=True, stop_on_consensus=False, **kw)


def test_engine_graph_path_obeys_bans():
    """A 16-token greedy decode through the graph path, then again with every token of the first
    run (its first token included) banned: none of them appears. Explicitly neutral values
    reproduce the unpenalised ids without capturing a second graph."""
    p = "Hallo tafel, wat is het plan voor vandaag?"
    e = eng(use_graphs=True)
    base = e.run_turns([Turn("K1", p, greedy())])[0]
    assert base.error is None and len(base.ids) == 16
    assert e.stats["graph_captures"] == 1
    neutral = e.run_turns([Turn("K2", p, greedy(repetition_penalty=1.0, repeat_last_n=64, presence_penalty=0.0,
                                                 frequency_penalty=0.0, logit_bias=None))])[0]
    assert neutral.ids == base.ids
    assert e.stats["graph_captures"] == 1 and len(e.graphs) == 1
    banned = e.run_turns([Turn("K3", p, greedy(logit_bias={a: -100.0 for a in set(base.ids)}))])[0]
    assert banned.error is None and len(banned.ids) == 16
    assert not set(banned.ids) & set(base.ids), (banned.ids, base.ids)
    assert e.stats["graph_captures"] == 2
    # the eager path applies the same op: same ids
    eager = eng(use_graphs=False).run_turns([Turn("K3", p, greedy(logit_bias={a: -100.0 for a in set(base.ids)}))])[0]
    assert eager.ids == banned.ids


def test_engine_mixed_batch_leaves_the_neutral_row():
    """One row with frequency_penalty 2 beside a neutral row, in the processors' graph: the neutral
    row's ids are those of the plain graph, and the penalised row's first token (nothing generated
    yet, repetition off) is the unpenalised one."""
    p = "Hallo tafel, wat is het plan voor vandaag?"
    e = eng(use_graphs=True)
    base = e.run_turns([Turn("K1", p, greedy()), Turn("K2", p + " Anders.", greedy())])
    both = e.run_turns([Turn("K1b", p, greedy()), Turn("K2b", p + " Anders.", greedy(frequency_penalty=2.0))])
    assert both[0].ids == base[0].ids
    assert both[1].error is None and both[1].ids[0] == base[1].ids[0]
    assert e.stats["graph_captures"] == 2
