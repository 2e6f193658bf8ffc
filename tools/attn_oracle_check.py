#!/usr/bin/env python3
"""Decode attention against the fp64 oracle in THIS process's environment.

    RT_ATTN_EXT_SPLITS=0 python tools/attn_oracle_check.py

The launch forms behind RT_ATTN_EXT_SPLITS, RT_ATTN_PP and RT_ATTN_LM (csrc/attn_plan.h knobs())
are chosen by an environment read that happens once per process, so each form needs a fresh
process: tests/test_attention_oracle_gpu.py starts this tool once per form. It runs a compact
list -- configs (32, 8, 128) and (8, 1, 128), splits 1 / 3 / 8, plain rows and the 3-member
shared-prefix table, kinds census, ramp (gaps 0.25 and 8) and random (ops/oracle64.py) -- with
and without the per-step plan, a second launch on the same workspace bit-equal to the first and
the arrival counters back at zero, and prints one JSON line with the worst error / tolerance per
case. Exit code 0 = every case inside its tolerance."""
from __future__ import annotations

import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from theroundtaible_amd import ops                      # noqa: E402
from theroundtaible_amd.ops import oracle64 as o64      # noqa: E402

CFGS = ((32, 8, 128), (8, 1, 128))
SPLITS = (1, 3, 8)
KINDS = ("census", "ramp_r025", "ramp_r8", "random")
KNOBS = ("RT_ATTN_EXT_SPLITS", "RT_ATTN_PP", "RT_ATTN_LM")


def main() -> int:
    dev = "cuda"
    assert torch.cuda.is_available() and ops.native_available()
    cases, bad = {}, []
    for hq, hkv, d in CFGS:
        G = hq // hkv
        for kind in KINDS:
            for layout, build in (("plain", o64.attn_decode_case), ("table3", o64.attn_table3_case)):
                case = build(kind, hq, hkv, d)
                e, A, tol = o64.attn_oracle(case)
                q, kc, vc, bt, cl = (t.to(dev) for t in (case.q, case.k_cache, case.v_cache, case.block_tables,
                                                         case.ctx_lens))
                groups = None
                if layout == "table3":
                    groups = ops.decode_groups(case.group_of, case.shared, G)[0].to(dev)
                for splits in SPLITS:
                    name = f"{hq}x{hkv}x{d} {kind} {layout} splits {splits}"
                    ws = ops.DecodeWorkspace(q.shape[0], hq, d, splits, dev, max_group=16 // G if groups is not None else 1)
                    out = ops.paged_attention_decode(q, kc, vc, bt, cl, case.scale, splits, ws, groups=groups)
                    again = ops.paged_attention_decode(q, kc, vc, bt, cl, case.scale, splits, ws, groups=groups)
                    ok = ops.attn_plan(bt, cl, splits, ws, hq, hkv, groups, q.shape[0])
                    planned = ops.paged_attention_decode(q, kc, vc, bt, cl, case.scale, splits, ws, groups=groups,
                                                         planned=True)
                    cases[name] = round(o64.error_ratio(out, e, tol), 4)
                    same = ok and torch.equal(out, again) and torch.equal(out, planned) and \
                        int(ws.counters.abs().sum()) == 0
                    if not (cases[name] <= 1.0 and same):
                        bad.append(name if same else name + " (relaunch / planned launch differs or counters left)")
    print(json.dumps({"attn_oracle_check": {k: os.environ.get(k) for k in KNOBS}, "worst": max(cases.values()),
                      "failed": bad, "cases": cases}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
