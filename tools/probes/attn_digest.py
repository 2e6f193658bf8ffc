#!/usr/bin/env python3
"""sha256 of the decode-attention output for fixed seeds, through the public ``ops`` API only.

    python tools/probes/attn_digest.py > digest.txt

Two trees that launch the same attention, plan and combine kernels with the same geometry print the
same listing line for line (the split combine merges in a fixed order). Only ``out`` is hashed: the
partial buffers hold uninitialised slots. Every case runs unplanned and with the per-step plan.
Shapes: those of tests/test_kernels_gpu.py (distinct rows, the ``table3`` and ``mixed`` shared-prefix
layouts) and one row with more tiles than a plan row holds. Under ``rocprofv3 --kernel-trace`` the
same run gives the launch geometry.
"""
import hashlib
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from theroundtaible_amd import ops  # noqa: E402

DEV = "cuda"


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def bf(g, *shape):
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(DEV)


def run(tag, hq, hkv, d, splits, spec):
    """spec: [(group label or None, shared blocks, [lengths])]; rows of one label share their first blocks."""
    g = torch.Generator(device="cpu").manual_seed(hq + 3 * hkv + 5 * d + 7 * splits + len(spec))
    lens = [l for _, _, ls in spec for l in ls]
    group_of = [label for label, _, ls in spec for _ in ls]
    shared = [sh for _, sh, ls in spec for _ in ls]
    B = len(lens)
    nb = sum(sh for _, sh, _ in spec) + sum((l + 31) // 32 for l in lens) + 4
    kc, vc = bf(g, nb, hkv, 32, d), bf(g, nb, hkv, d, 32)
    perm = torch.randperm(nb, generator=g).tolist()
    bt = torch.zeros(B, max((l + 31) // 32 for l in lens), dtype=torch.int32)
    nxt = b = 0
    for _, sh, ls in spec:
        common = perm[nxt:nxt + sh]
        nxt += sh
        for l in ls:
            own = (l + 31) // 32 - sh
            bt[b, :sh + own] = torch.tensor(common + perm[nxt:nxt + own], dtype=torch.int32)
            nxt += own
            b += 1
    G = hq // hkv
    grouped = any(label is not None for label in group_of)
    groups = ops.decode_groups(group_of, shared, G)[0].to(DEV) if grouped else None
    q = bf(g, B, hq, d)
    bt, cl = bt.to(DEV), torch.tensor(lens, dtype=torch.int32).to(DEV)
    ws = ops.DecodeWorkspace(B, hq, d, splits, DEV, max_group=16 // G if grouped else 1)
    scale = 1 / math.sqrt(d)
    out = ops.paged_attention_decode(q, kc, vc, bt, cl, scale, splits, ws, groups=groups)
    print(f"{tag} Hq={hq} Hkv={hkv} D={d} splits={splits} unplanned {sha(out)}", flush=True)
    assert ops.attn_plan(bt, cl, splits, ws, hq, hkv, groups, B)
    out = ops.paged_attention_decode(q, kc, vc, bt, cl, scale, splits, ws, groups=groups, planned=True)
    print(f"{tag} Hq={hq} Hkv={hkv} D={d} splits={splits} planned {sha(out)}", flush=True)


def main() -> None:
    rows = [(None, 0, [l]) for l in [1, 31, 32, 33, 257, 1500]]
    table3 = [("A", 1900 // 32, [1900 + 7, 1900 + 300, 1900 + 33])]
    mixed = [("A", 40, [40 * 32 + 1, 40 * 32 + 500]), (None, 0, [700]),
             ("B", 3, [3 * 32 + 5, 96 + 64, 96 + 1, 96 + 900])]
    shapes = [(32, 8, 128), (64, 8, 128), (12, 12, 64), (4, 1, 128), (28, 4, 128)]
    for hq, hkv, d in shapes:
        for splits in (1, 3, 8, 64):
            run("rows", hq, hkv, d, splits, rows)
    for name, spec in (("table3", table3), ("mixed", mixed)):
        for hq, hkv, d in shapes:
            for splits in (1, 3, 10, 64):
                run(name, hq, hkv, d, splits, spec)
    run("long", 32, 8, 128, 1, [(None, 0, [20000])])   # 625 tiles: more than a plan row's 512 ids
    torch.cuda.synchronize()
    print("done", flush=True)


if __name__ == "__main__":
    main()
