"""The logit processors' semantics (ops/reference.py, the CPU fallback of csrc/logit_proc.hip) rule
by rule against hand-computed values and against the independent fp64 oracle (ops/oracle64.py)."""
import pytest
import torch

from theroundtaible_amd import ops
from theroundtaible_amd.ops import oracle64 as o64

V = 32
W = ops.LOGIT_PROC_WINDOW


def make(hist=(), reply_from=0, rp=1.0, last_n=64, pp=0.0, fp=0.0, bias=None, cap=None):
    """A one-row proc."""
    p = ops.LogitProc(1, "cpu", hist_cap=cap or max(len(hist), 1))
    p.hist[0, :len(hist)] = torch.tensor(list(hist), dtype=torch.int32)
    p.hist_len[0] = len(hist)
    p.reply_from[0] = reply_from
    p.rp[0], p.last_n[0], p.pp[0], p.fp[0] = rp, last_n, pp, fp
    for j, (t, v) in enumerate((bias or {}).items() if isinstance(bias, dict) else (bias or [])):
        p.bias_tok[0, j], p.bias_val[0, j] = t, v
        p.bias_n[0] = j + 1
    return p


def run(logits, proc, out=None, step=None):
    """Reference result, checked against the oracle (named within tolerance, the rest bit-equal)."""
    got = ops.apply_logit_processors(logits.clone(), proc, out, step)
    e, mag, named = o64.apply_logit_processors(logits, proc, out, step)
    o64.assert_within(got, e, o64.logit_proc_tol(e, mag, logits.dtype), dtype=logits.dtype)
    view = torch.int16 if logits.dtype == torch.bfloat16 else torch.int32
    assert torch.equal(got.view(view)[~named], logits.view(view)[~named])
    return got, named


def row(**at):
    lg = torch.linspace(-2.0, 2.0, V).reshape(1, V).clone()
    for t, v in at.items():
        lg[0, int(t[1:])] = v
    return lg


def changed(got, lg):
    return sorted((got != lg).nonzero()[:, 1].tolist())


def test_repetition_penalty_divides_positive_and_multiplies_negative():
    lg = row(t3=2.0, t4=-2.0, t5=0.0)
    got, _ = run(lg, make(hist=[3, 4, 5], rp=2.0))
    assert got[0, 3] == 1.0 and got[0, 4] == -4.0 and got[0, 5] == 0.0
    assert changed(got, lg) == [3, 4]


def test_repetition_covers_the_prompt_presence_and_frequency_only_the_reply():
    lg = row(t1=1.0, t2=1.0)
    got, _ = run(lg, make(hist=[1, 2, 2], reply_from=1, rp=2.0, pp=0.25, fp=0.5))
    assert got[0, 1] == 0.5                         # prompt token: repetition only
    assert got[0, 2] == 0.5 - 0.5 * 2 - 0.25        # reply token, twice
    assert changed(got, lg) == [1, 2]


def test_order_bias_then_repetition_then_frequency_and_presence():
    lg = row(t7=-1.0)
    got, _ = run(lg, make(hist=[7], rp=2.0, pp=0.25, fp=0.5, bias={7: 3.0}))
    assert got[0, 7] == (-1.0 + 3.0) / 2.0 - 0.5 - 0.25     # the bias made it positive: divided
    lg = row(t7=1.0)
    got, _ = run(lg, make(hist=[7], rp=2.0, bias={7: -3.0}))
    assert got[0, 7] == (1.0 - 3.0) * 2.0


def test_bias_alone_and_its_limits():
    lg = row()
    got, named = run(lg, make(bias={0: -100.0, 31: 100.0, 9: 0.0}))
    assert got[0, 0] == lg[0, 0] - 100.0 and got[0, 31] == lg[0, 31] + 100.0
    assert sorted(named[0].nonzero().flatten().tolist()) == [0, 9, 31]
    # ids outside [0, V) are ignored; a token named twice keeps its last entry
    got, _ = run(lg, make(bias=[(-1, 5.0), (V, 5.0), (4, 1.0), (4, 2.0)]))
    assert changed(got, lg) == [4] and got[0, 4] == lg[0, 4] + 2.0


def test_repeat_last_n_window_zero_and_minus_one():
    lg = row(t1=1.0, t2=1.0, t3=1.0)
    hist = [1, 2, 3, 3]
    assert changed(run(lg, make(hist=hist, rp=2.0, last_n=2))[0], lg) == [3]
    assert changed(run(lg, make(hist=hist, rp=2.0, last_n=3))[0], lg) == [2, 3]
    assert changed(run(lg, make(hist=hist, rp=2.0, last_n=0))[0], lg) == []
    assert changed(run(lg, make(hist=hist, rp=2.0, last_n=-1))[0], lg) == [1, 2, 3]
    assert changed(run(lg, make(hist=hist, rp=2.0, last_n=10 ** 6))[0], lg) == [1, 2, 3]


def test_window_cuts_inside_the_host_part():
    """3000 host tokens: only the last 2048 count, for the repetition set (last_n = -1) and for
    the reply (reply_from = 0)."""
    hist = [1] * 952 + [2] * 2048
    lg = row(t1=1.0, t2=1.0)
    got, _ = run(lg, make(hist=hist, rp=2.0, last_n=-1))
    assert changed(got, lg) == [2]
    got, _ = run(lg, make(hist=[1] * 953 + [2] * 2047, rp=2.0, last_n=-1))
    assert changed(got, lg) == [1, 2]
    got, _ = run(lg, make(hist=hist, fp=2.0 ** -12))
    assert changed(got, lg) == [2] and got[0, 2] == 1.0 - 2048 * 2.0 ** -12
    got, _ = run(lg, make(hist=[1] * 953 + [2] * 2047, fp=2.0 ** -12))
    assert got[0, 1] == 1.0 - 2.0 ** -12 and got[0, 2] == 1.0 - 2047 * 2.0 ** -12


def test_window_cuts_inside_the_device_part():
    """5 host tokens and 2500 device tokens: the window starts inside ``out``."""
    out = torch.zeros(2600, 1, dtype=torch.int64)
    out[:452, 0] = 3
    out[452:2500, 0] = 4
    out[2500:, 0] = 5                               # beyond ``step``: never read
    step = torch.tensor([2500])
    lg = row(t1=1.0, t3=1.0, t4=1.0, t5=1.0)
    got, _ = run(lg, make(hist=[1] * 5, rp=2.0, last_n=-1, fp=2.0 ** -12), out, step)
    assert changed(got, lg) == [4] and got[0, 4] == 0.5 - 2048 * 2.0 ** -12
    got, _ = run(lg, make(hist=[1] * 5, rp=2.0, last_n=-1, fp=2.0 ** -12), out, torch.tensor([2499]))
    assert changed(got, lg) == [3, 4] and got[0, 3] == 0.5 - 2.0 ** -12 and got[0, 4] == 0.5 - 2047 * 2.0 ** -12
    # step 0 and no step: the host part alone
    for o, s in ((out, torch.tensor([0])), (None, None)):
        got, _ = run(lg, make(hist=[1] * 5, rp=2.0, last_n=-1), o, s)
        assert changed(got, lg) == [1]


def test_token_in_both_parts_and_duplicates():
    out = torch.tensor([[6], [6], [8]], dtype=torch.int64)
    lg = row(t6=2.0, t8=2.0)
    got, _ = run(lg, make(hist=[6, 9, 6], reply_from=2, pp=0.25, fp=0.5), out, torch.tensor([3]))
    assert got[0, 6] == 2.0 - 0.5 * 3 - 0.25        # once in the host reply, twice on the device
    assert got[0, 8] == 2.0 - 0.5 - 0.25
    assert changed(got, lg) == [6, 8]               # 9 and the first 6 precede the reply


def test_device_tokens_all_belong_to_the_reply():
    out = torch.tensor([[2], [2]], dtype=torch.int64)
    lg = row(t2=1.0)
    got, _ = run(lg, make(hist=[2, 2], reply_from=2, fp=0.25), out, torch.tensor([2]))
    assert got[0, 2] == 0.5
    got, _ = run(lg, make(hist=[2, 2], reply_from=99, fp=0.25), out, torch.tensor([2]))   # clamped to the host part
    assert got[0, 2] == 0.5


def test_out_of_range_history_ids_are_ignored():
    out = torch.tensor([[-5], [V], [2 ** 40], [1]], dtype=torch.int64)
    lg = row(t1=1.0)
    got, named = run(lg, make(hist=[-1, V, V + 100, 2 ** 31 - 1], rp=2.0, fp=0.5), out, torch.tensor([4]))
    assert changed(got, lg) == [1] and int(named.sum()) == 1


def test_minus_infinity_stays():
    lg = row(t1=float("-inf"), t2=float("-inf"))
    got, _ = run(lg, make(hist=[1], rp=2.0, pp=-2.0, fp=-2.0, bias={1: 100.0, 2: 100.0}))
    assert got[0, 1] == float("-inf") and got[0, 2] == float("-inf")
    assert torch.equal(got[0, 3:], lg[0, 3:])


def test_neutral_rows_keep_their_bits():
    lg = torch.randn(3, V, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    proc = ops.LogitProc(3, "cpu", hist_cap=8)
    proc.hist[:] = torch.arange(8, dtype=torch.int32)
    proc.hist_len.fill_(8)
    proc.rp[1] = 1.5
    proc.last_n.copy_(torch.tensor([64, 64, 0], dtype=torch.int32))
    proc.rp[2] = 1.5                                # repetition switched off by last_n = 0: neutral
    got, named = run(lg, proc)
    assert not bool(named[0].any()) and not bool(named[2].any()) and int(named[1].sum()) == 8
    assert torch.equal(got[0].view(torch.int16), lg[0].view(torch.int16))
    assert torch.equal(got[2].view(torch.int16), lg[2].view(torch.int16))


def test_bf16_result_is_rounded_once():
    lg = torch.full((1, V), 1.0, dtype=torch.bfloat16)
    got, _ = run(lg, make(hist=[3], rp=3.0, fp=0.3, pp=0.1, bias={3: 0.7}))
    want = torch.tensor(1.0) + torch.tensor(0.7)
    want = want / torch.tensor(3.0) - torch.tensor(0.3) * torch.tensor(1.0) - torch.tensor(0.1)
    assert got[0, 3] == want.to(torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("Vc", o64.LOGIT_PROC_V)
def test_reference_matches_oracle_on_the_gpu_test_inputs(Vc, dtype):
    """The inputs of tests/test_logit_proc_gpu.py: the CPU fallback meets the kernel's bound."""
    for n_hist in o64.LOGIT_PROC_HIST:
        for step in o64.LOGIT_PROC_STEPS:
            logits, proc, out, st = o64.logit_proc_case(Vc, dtype, n_hist, step)
            _, named = run(logits, proc, out, st)
            assert not bool(named[0].any()) and bool(named[2].any())


def test_fill_keeps_the_tail_and_moves_the_reply_start():
    from theroundtaible_amd.engine import SamplingParams
    p = SamplingParams(frequency_penalty=1.0, logit_bias={5: -100.0, 6: 2.0})
    proc = ops.LogitProc(3, "cpu", hist_cap=4)
    proc.fill([(list(range(10)), 8, p), None, (list(range(3)), 1, SamplingParams())])
    assert proc.active
    assert proc.hist[0].tolist() == [6, 7, 8, 9] and int(proc.hist_len[0]) == 4 and int(proc.reply_from[0]) == 2
    assert int(proc.bias_n[0]) == 2 and proc.bias_tok[0, :2].tolist() == [5, 6]
    assert proc.rp.tolist() == [1.0, 1.0, 1.0] and int(proc.hist_len[2]) == 0     # neutral params: neutral row
    proc.fill([(list(range(10)), 2, p), None, None])                               # the reply began before the tail
    assert int(proc.reply_from[0]) == 0
    assert not proc.fill([None, None, None]).active
