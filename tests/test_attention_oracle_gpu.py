"""The attention kernels (K3 decode: csrc/attn_core.h, attention_decode.hip, attn_plan.h; K4 prefill:
attention_prefill32.hip, attention_prefill.hip and the key-split combine) against the fp64 oracle of
ops/oracle64.py, every output element within ``attn_tol``: one bf16 ulp plus the bf16 rounding of P
(2^-8 of the weighted |V|; nothing for the census inputs, whose p are all exactly 1) plus the measured
fp32 slack. Inputs (random, peaky, census markers, score ramps, one-hot keys; finite poison in every
slot past a row's end, in every unreferenced block and behind every block-table padding entry) come
from the builders the CPU test (tests/test_attention_oracle_cpu.py) proves sound and sharp."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from theroundtaible_amd import ops
from theroundtaible_amd.ops import oracle64 as o64

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class OnDevice:
    def __init__(self, case, prefill=False):
        self.case = case
        self.e, self.A, self.tol = o64.attn_oracle(case, prefill)
        self.q, self.kc, self.vc, self.bt, self.cl, self.cu, self.st = (
            t.to(DEV) for t in (case.q, case.k_cache, case.v_cache, case.block_tables, case.ctx_lens, case.cu_q,
                                case.start_pos))


@functools.lru_cache(maxsize=2)
def decode_case(kind, cfg, lens=o64.ATTN_DECODE_LENS):
    return OnDevice(o64.attn_decode_case(kind, *cfg, lens=lens))


@functools.lru_cache(maxsize=2)
def group_case(kind, cfg):
    return OnDevice(o64.attn_group_case(kind, *cfg))


@functools.lru_cache(maxsize=2)
def prefill_case(kind, cfg, specs):
    return OnDevice(o64.attn_case(kind, *cfg, specs), prefill=True)


def check_decode(c, splits, what, grouped=False):
    """One launch within the tolerance; a second launch on the same workspace and the planned launch
    reproduce it bit for bit and leave the arrival counters at zero."""
    case = c.case
    hq, hkv, d = case.hq, case.hkv, case.d
    G = hq // hkv
    B = c.q.shape[0]
    groups = None
    if grouped:
        table, nmax = ops.decode_groups(case.group_of, case.shared, G)
        assert nmax <= max(1, 16 // G)
        groups = table.to(DEV)
    ws = ops.DecodeWorkspace(B, hq, d, splits, DEV, max_group=16 // G if grouped else 1)
    out = ops.paged_attention_decode(c.q, c.kc, c.vc, c.bt, c.cl, case.scale, splits, ws, groups=groups)
    r = o64.assert_within(out, c.e, c.tol, what)
    print(f"{what}: error / tolerance {r:.3f}")
    again = ops.paged_attention_decode(c.q, c.kc, c.vc, c.bt, c.cl, case.scale, splits, ws, groups=groups)
    assert torch.equal(out, again)
    assert int(ws.counters.abs().sum()) == 0
    assert ops.attn_plan(c.bt, c.cl, splits, ws, hq, hkv, groups, B)
    planned = ops.paged_attention_decode(c.q, c.kc, c.vc, c.bt, c.cl, case.scale, splits, ws, groups=groups,
                                         planned=True)
    o64.assert_within(planned, c.e, c.tol, what + " planned")
    assert torch.equal(out, planned)
    assert int(ws.counters.abs().sum()) == 0
    return r


@pytest.mark.parametrize("splits", o64.ATTN_DECODE_SPLITS)
@pytest.mark.parametrize("kind", o64.ATTN_KINDS)
@pytest.mark.parametrize("cfg", o64.ATTN_DECODE_CFGS)
def test_decode(cfg, kind, splits):
    """GM 4 / 8 / 16, both K/V loop forms under the default rule, G = 7, D = 64; contexts on and
    around the 32-key tile; at 64 splits most items are empty."""
    check_decode(decode_case(kind, cfg), splits, f"decode {cfg} {kind} splits {splits}")


@pytest.mark.parametrize("splits", o64.ATTN_REFILL_SPLITS)
@pytest.mark.parametrize("kind", o64.ATTN_REFILL_KINDS)
@pytest.mark.parametrize("cfg", o64.ATTN_REFILL_CFGS)
def test_decode_refill_and_plan_row_boundary(cfg, kind, splits):
    """16417 keys (tile 512 full, tile 513 partial): the smallest row that reaches the per-lane
    block-id refill (tile index j & 63 == 0 again) and the plan row's 512-tile limit; marks on keys
    16351, 16352, 16383, 16384 and 16416."""
    marks = o64.attn_marks(o64.ATTN_REFILL_LENS[0])
    assert {16351, 16352, 16383, 16384, 16416} <= set(marks)
    check_decode(decode_case(kind, cfg, o64.ATTN_REFILL_LENS), splits, f"refill {cfg} {kind} splits {splits}")


@pytest.mark.parametrize("splits", o64.ATTN_GROUP_SPLITS)
@pytest.mark.parametrize("kind", o64.ATTN_KINDS)
@pytest.mark.parametrize("cfg", o64.ATTN_GROUP_CFGS)
def test_grouped_decode(cfg, kind, splits):
    """Shared-prefix groups (ATTN_GROUP_LAYOUT), every row against the oracle of that sequence alone."""
    check_decode(group_case(kind, cfg), splits, f"grouped {cfg} {kind} splits {splits}", grouped=True)


def test_prefill_rows_per_tile_agree():
    for hq, hkv, d in o64.ATTN_PREFILL_CFGS + o64.ATTN_SPLIT_CFGS:
        assert o64.attn_prefill_rows(hq // hkv, d) == ops.native().prefill_rows_per_tile(hq // hkv, d)


@pytest.mark.parametrize("kind", o64.ATTN_KINDS)
@pytest.mark.parametrize("cfg", o64.ATTN_PREFILL_CFGS)
def test_prefill(cfg, kind):
    """The 32x32 kernel (padded head slots at G = 7 and 3), the 16x16 kernel; chunks on and around the
    64-key tile edge of the whole-tile-visible test. census pins every row's causal limit."""
    c = prefill_case(kind, cfg, o64.ATTN_PREFILL_SPECS)
    out = ops.prefill_attention(c.q, c.kc, c.vc, c.bt, c.cu, c.st, c.case.scale)
    r = o64.assert_within(out, c.e, c.tol, f"prefill {cfg} {kind}")
    print(f"prefill {cfg} {kind}: error / tolerance {r:.3f}")
    assert torch.equal(out, ops.prefill_attention(c.q, c.kc, c.vc, c.bt, c.cu, c.st, c.case.scale))


@pytest.mark.parametrize("min_chunk", o64.ATTN_SPLIT_MIN_CHUNK)
@pytest.mark.parametrize("kind", o64.ATTN_KINDS)
@pytest.mark.parametrize("cfg", o64.ATTN_SPLIT_CFGS)
def test_prefill_key_split(cfg, kind, min_chunk):
    c = prefill_case(kind, cfg, o64.ATTN_SPLIT_SPECS)
    case = c.case
    rows = ops.native().prefill_rows_per_tile(case.hq // case.hkv, case.d)
    plan = ops.prefill_split_plan(case.cu_q, rows, case.start_pos, case.hkv, num_cus=1 << 20, min_chunk_tiles=min_chunk)
    assert plan is not None and plan[2] >= 2
    split = (plan[0].to(DEV), plan[1].to(DEV), plan[2])
    what = f"key split {cfg} {kind} chunk {min_chunk}"
    out = ops.prefill_attention(c.q, c.kc, c.vc, c.bt, c.cu, c.st, case.scale, split=split)
    r = o64.assert_within(out, c.e, c.tol, what)
    print(f"{what}: error / tolerance {r:.3f}")
    whole = ops.prefill_attention(c.q, c.kc, c.vc, c.bt, c.cu, c.st, case.scale)
    o64.assert_within(whole, c.e, c.tol, what + " whole tiles")
    # two results inside the tolerance of one oracle are within twice it of each other
    o64.assert_within(out, whole.cpu().double(), 2 * c.tol, what + " vs whole tiles")
    assert torch.equal(out, ops.prefill_attention(c.q, c.kc, c.vc, c.bt, c.cu, c.st, case.scale, split=split))


@pytest.mark.parametrize("env", [{"RT_ATTN_EXT_SPLITS": "0"}, {"RT_ATTN_PP": "0"}, {"RT_ATTN_PP": "1"},
                                 {"RT_ATTN_LM": "7"}], ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_decode_knob_forms(env):
    """The launch forms chosen by a process-static environment read (csrc/attn_plan.h knobs()): the
    in-launch combine at 2 or more splits, both K/V loop forms pinned, the LDS-DMA staged loop; each
    in a fresh child process running tools/attn_oracle_check.py."""
    cmd = [sys.executable, os.path.join(ROOT, "tools", "attn_oracle_check.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, **env), cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"attn_oracle_check"')]
    assert len(recs) == 1, r.stdout[-2000:]
    rec = recs[0]
    assert all(rec["attn_oracle_check"][k] == v for k, v in env.items())
    assert rec["failed"] == [] and rec["worst"] <= 1.0 and len(rec["cases"]) == 2 * 4 * 2 * 3, rec
    print(f"{env}: worst error / tolerance {rec['worst']}")
