#!/usr/bin/env python3
"""Probe: decode attention + combine per call with a bf16 and an fp8 K/V cache (kv_dtype "fp8") at the
shapes of profiles/r14/kv_fp8/README.md section 2: 3 knights x 22K / 40K shared keys (grouped), B = 1 at
25K, B = 16 at 2K; Llama-3-8B heads, the engine's split rule, planned launches. hipGraph replays of 20
calls over 6 rotating cache copies, best of 7, every case and dtype twice in alternation. One JSON line
per measurement ("attn_fp8_bench": the tag); the refit t = a + bytes / rate is a least-squares line
through the smaller time of each case.

    python tools/probes/attn_kv_fp8.py <tree root> <bf16|bf16,fp8> <tag>

<tree root>: the checkout whose extension is timed ("." here; a built checkout of the parent commit for
its bf16 numbers, which takes "bf16" only)."""
import json
import math
import os
import sys

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tools"))
import torch  # noqa: E402
from theroundtaible_amd import ops  # noqa: E402
from microbench import timed  # noqa: E402

DEV = "cuda"
dtypes = sys.argv[2].split(",")
tag = sys.argv[3]
hq, hkv, d = 32, 8, 128
G = hq // hkv


def cache(nblk, kv):
    if kv == "fp8":
        # random finite e4m3 codes (exponent field < 15 keeps every byte finite)
        k = torch.randint(0, 120, (nblk, hkv, 32, d), device=DEV, dtype=torch.uint8)
        v = torch.randint(0, 120, (nblk, hkv, d, 32), device=DEV, dtype=torch.uint8)
        return k, v
    return ((torch.randn(nblk, hkv, 32, d, device=DEV)).to(torch.bfloat16),
            (torch.randn(nblk, hkv, d, 32, device=DEV)).to(torch.bfloat16))


def run(name, B, bt, cl, groups, nblk, keys_read, kv):
    copies = 6
    caches = [cache(nblk, kv) for _ in range(copies)]
    q = torch.randn(B, hq, d, device=DEV).to(torch.bfloat16)
    splits = ops.decode_splits(B, hkv, grouped=groups is not None)
    ws = ops.DecodeWorkspace(B, hq, d, splits, DEV, max_group=16 // G if groups is not None else 1)
    out = torch.empty_like(q)
    pl = ops.attn_plan(bt, cl, splits, ws, hq, hkv, groups, B)
    kw = dict(k_scale=0.5, v_scale=2.0) if kv == "fp8" else {}
    fn = lambda i: ops.paged_attention_decode(q, caches[i % copies][0], caches[i % copies][1], bt, cl,   # noqa: E731
                                              1 / math.sqrt(d), splits, ws, out, groups=groups, planned=pl, **kw)
    us = timed(fn, iters=20, reps=7)
    nbytes = keys_read * hkv * d * 2 * (1 if kv == "fp8" else 2)
    rec = {"attn_fp8_bench": tag, "case": name, "kv": kv, "splits": splits, "us": round(us, 2), "bytes": nbytes,
           "TBps": round(nbytes / us / 1e6, 3)}
    print(json.dumps(rec), flush=True)
    del caches


def grouped(shared, private=1500, B=3):
    nsh, npr = shared // 32, (private + 31) // 32
    nblk = nsh + B * npr
    bt = torch.zeros(B, nsh + npr, dtype=torch.int32)
    for b in range(B):
        bt[b, :nsh] = torch.arange(nsh)
        bt[b, nsh:] = nsh + b * npr + torch.arange(npr)
    cl = torch.full((B,), nsh * 32 + private, device=DEV, dtype=torch.int32)
    groups, _ = ops.decode_groups(["g"] * B, [nsh] * B, G)
    return B, bt.to(DEV), cl, groups.to(DEV), nblk, nsh * 32 + B * private


def private(B, ctx):
    nblk = (ctx + 31) // 32
    bt = torch.arange(B * nblk, device=DEV, dtype=torch.int32).reshape(B, nblk)
    cl = torch.full((B,), ctx, device=DEV, dtype=torch.int32)
    return B, bt, cl, None, B * nblk, B * ctx


CASES = [("3 knights x 22K shared + 1500 own (grouped)", grouped(22000)),
         ("3 knights x 40K shared + 1500 own (grouped)", grouped(40000)),
         ("B=1 ctx 25K", private(1, 25000)), ("B=16 ctx 2K", private(16, 2000))]
for rep in range(2):                       # alternating: every case, every dtype, twice
    for name, (B, bt, cl, groups, nblk, keys) in CASES:
        for kv in dtypes:
            run(name, B, bt, cl, groups, nblk, keys, kv)
