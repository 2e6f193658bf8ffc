#!/usr/bin/env python3
"""Probe: the five Llama-3-8B decode GEMMs at M rows, bf16 weights vs fp8 weights (e4m3 codes +
per-row scales, csrc/gemm_skinny_fp8.hip) vs mxfp4 weights (e2m1 codes + one e8m0 scale byte per
32 k, csrc/gemm_skinny_fp4.hip), alternating in one process so all three see the same box.
The bf16 calls are the ones the engine makes (split workspace and modes of
LlamaModel.forward_decode_fused). Same harness as tools/microbench.py (hipGraph of 20 calls,
>= 1 GiB of rotating weight copies, so every call reads cold weights). Prints us per call, the
weight bytes of one call and the rate they stream at.

    python tools/probes/gemm_mxfp4.py [--rows 3] [--rounds 3]
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from microbench import bf, timed  # noqa: E402
from theroundtaible_amd import ops  # noqa: E402
from theroundtaible_amd.ops import reference as ref  # noqa: E402

DEV = "cuda"


def run(M: int, rounds: int):
    hid, ffn, hq, hkv, d, vocab = 4096, 14336, 32, 8, 128, 128256
    x, res, g_in = bf(M, hid), bf(M, hid), bf(M, ffn)
    nb = 64
    kc = torch.zeros(nb, hkv, 32, d, dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros(nb, hkv, d, 32, dtype=torch.bfloat16, device=DEV)
    cs = ref.rope_cos_sin(8192, d, 500000.0, DEV)
    pos = torch.arange(M, device=DEV, dtype=torch.int64) + 100
    slots = torch.arange(M, device=DEV, dtype=torch.int64) + 40
    sw, SK, ALL = ops.split_workspace(DEV), ops.SPLIT_K, ops.SPLIT_K | ops.SPLIT_BALANCE
    rope = dict(rope_heads=hq + hkv, head_dim=d)

    def qkv(W, s, ws, mode):
        return ops.skinny_gemm_rope(x, W, ops.PRO_NORM, pos, cs, kc, vc, slots, hq, hkv, d, split_ws=ws,
                                    split_mode=mode, wscale=s)

    # name, weight rows, K, shuffle kwargs, call(W, scale, split_ws, split_mode), the engine's bf16 split mode
    shapes = [
        ("qkv (norm+rope+cache)", (hq + 2 * hkv) * d, hid, rope, qkv, SK),
        ("o (+resid)", hid, hq * d, {},
         lambda W, s, ws, mode: ops.skinny_gemm(x, W, ops.PRO_PLAIN, ops.EPI_RESID, res=res, split_ws=ws,
                                                split_mode=mode, wscale=s), SK),
        ("gate_up (norm+swiglu)", 2 * ffn, hid, {"swiglu": True},
         lambda W, s, ws, mode: ops.skinny_gemm(x, W, ops.PRO_NORM, ops.EPI_SWIGLU, split_ws=ws, split_mode=mode,
                                                wscale=s), ALL),
        ("down (+resid)", hid, ffn, {},
         lambda W, s, ws, mode: ops.skinny_gemm(g_in, W, ops.PRO_PLAIN, ops.EPI_RESID, res=res, split_ws=ws,
                                                split_mode=mode, wscale=s), SK),
        ("lm_head (norm)", vocab, hid, {},
         lambda W, s, ws, mode: ops.skinny_gemm(x, W, ops.PRO_NORM, ops.EPI_STORE, split_ws=ws, split_mode=mode,
                                                wscale=s), SK),
    ]
    for name, N, K, kw, call, mode in shapes:
        copies = max(2, math.ceil(2**30 / (N * K * 2)))
        W16, W8, W4 = [], [], []
        for _ in range(copies):
            W = bf(N, K, scale=0.02)
            W16.append(ops.shuffle_weight(W, **kw))
            W8.append(ops.shuffle_weight_fp8(W, **kw))
            W4.append(ops.shuffle_weight_mxfp4(W, **kw))
            del W
        for r in range(rounds):
            t16 = timed(lambda i: call(W16[i % copies], None, sw, mode))
            t8 = timed(lambda i: call(W8[i % copies][0], W8[i % copies][1], None, 0))
            t4 = timed(lambda i: call(W4[i % copies][0], W4[i % copies][1], None, 0))
            b16, b8, b4 = N * K * 2, N * K + N * 4, N * K // 2 + N * K // 32
            print(f"M={M} {name:24s} N={N:6d} K={K:5d} round {r}: bf16 {t16:7.2f} us ({b16 / 2**20:7.1f} MiB, "
                  f"{b16 / t16 / 1e6:4.2f} TB/s) | fp8 {t8:7.2f} us ({b8 / 2**20:7.1f} MiB, {b8 / t8 / 1e6:4.2f} TB/s) "
                  f"| mxfp4 {t4:7.2f} us ({b4 / 2**20:7.1f} MiB, {b4 / t4 / 1e6:4.2f} TB/s) "
                  f"| fp8 / bf16 = {t8 / t16:.3f} | mxfp4 / fp8 = {t4 / t8:.3f}", flush=True)
        del W16, W8, W4
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    torch.manual_seed(0)
    run(a.rows, a.rounds)
