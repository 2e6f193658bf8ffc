#!/usr/bin/env python3
"""sha256 of every decode-GEMM form's output for fixed seeds, through the public ``ops`` API only.

    python tools/probes/gemm_digest.py > digest.txt

Two trees that launch the same kernels with the same geometry on the same weights print the same
listing line for line (every form is deterministic: split parts are summed in index order). Each
line is one buffer: the GEMM output (``out`` / ``res`` / ``q``), the K/V caches of a ROPE row, and
the shuffled or quantised weight buffers (and their unshuffled copies at the small shapes).
Shapes: the Llama-3-8B decode / shard / serving-batch rows that csrc/tests/host_check.cpp plans,
then the smallest shape of each form. Under ``rocprofv3 --kernel-trace`` the same run gives the
launch geometry.
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from theroundtaible_amd import ops  # noqa: E402
from theroundtaible_amd.ops import reference as ref  # noqa: E402

DEV = "cuda"
PLAIN, NORM, NORM_ADD = ops.PRO_PLAIN, ops.PRO_NORM, ops.PRO_NORM_ADD
STORE, RESID, SWIGLU, ROPE = ops.EPI_STORE, ops.EPI_RESID, ops.EPI_SWIGLU, ops.EPI_ROPE
PRO = {PLAIN: "plain", NORM: "norm", NORM_ADD: "norm_add"}
EPI = {STORE: "store", RESID: "resid", SWIGLU: "swiglu", ROPE: "rope"}


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def emit(tag: str, name: str, t: torch.Tensor) -> None:
    print(f"{tag} {name} {sha(t)}", flush=True)


_weights = {}


def weight(fp8: bool, n: int, k: int, pro: int, epi: int, heads):
    """(Ws, wscale) of an [n, k] decode weight (SwiGLU: [2n, k]); built and printed once per kind."""
    key = (fp8, n, k, pro != PLAIN, epi == SWIGLU, heads)
    if key not in _weights:
        g = torch.Generator(device="cpu").manual_seed(1000 + n + 7 * k)
        rows = 2 * n if epi == SWIGLU else n
        W = (torch.randn(rows, k, generator=g, dtype=torch.float32) * 0.05).to(torch.bfloat16).to(DEV)
        gamma = (1 + 0.1 * torch.randn(k, generator=g)).to(torch.bfloat16).to(DEV) if pro != PLAIN else None
        rh, d = (heads[0] + heads[1], heads[2]) if heads else (0, 0)
        tag = f"weight {'fp8' if fp8 else 'bf16'} {rows}x{k} gamma={int(gamma is not None)} rope={rh} swiglu={int(epi == SWIGLU)}"
        if fp8:
            Wq, sc = ops.shuffle_weight_fp8(W, gamma, rh, d, epi == SWIGLU)
            emit(tag, "codes", Wq)
            emit(tag, "scale", sc)
            if rows * k <= 1 << 24:
                emit(tag, "unshuffled", ops.unshuffle_weight_fp8(Wq, sc, rh, d, epi == SWIGLU))
            _weights[key] = (Wq, sc)
        else:
            Ws = ops.shuffle_weight(W, gamma, rh, d, epi == SWIGLU)
            emit(tag, "shuffled", Ws)
            if rows * k <= 1 << 24:
                emit(tag, "unshuffled", ops.unshuffle_weight(Ws, rh, d, epi == SWIGLU))
            _weights[key] = (Ws, None)
        del W
    return _weights[key]


def run(fp8: bool, m: int, n: int, k: int, pro: int, epi: int, split_mode: int, ws, heads=None) -> None:
    tag = (f"{'fp8' if fp8 else 'bf16'} M={m} N={n} K={k} {PRO[pro]} {EPI[epi]} split_mode={split_mode} "
           f"ws={int(ws is not None)}")
    Ws, sc = weight(fp8, n, k, pro, epi, heads)
    g = torch.Generator(device="cpu").manual_seed(m + 3 * n + 5 * k + 11 * pro + 13 * epi)
    x = torch.randn(m, k, generator=g).to(torch.bfloat16).to(DEV)
    kw = dict(wscale=sc) if fp8 else dict(split_ws=ws, split_mode=split_mode)
    if pro == NORM_ADD:
        kw["x2"] = torch.randn(m, k, generator=g).to(torch.bfloat16).to(DEV)
        kw["xout"] = torch.empty_like(x)
    if epi == ROPE:
        hq, hkv, d = heads
        nb = 8
        cos_sin = ref.rope_cos_sin(4096, d, 500000.0, DEV)
        positions = torch.randint(0, 4000, (m,), generator=g, dtype=torch.int64).to(DEV)
        slots = torch.randperm(nb * 32, generator=g)[:m].to(torch.int64).to(DEV)
        kc = torch.zeros(nb, hkv, 32, d, dtype=torch.bfloat16, device=DEV)
        vc = torch.zeros(nb, hkv, d, 32, dtype=torch.bfloat16, device=DEV)
        q = ops.skinny_gemm_rope(x, Ws, pro, positions, cos_sin, kc, vc, slots, hq, hkv, d, **kw)
        emit(tag, "q", q)
        emit(tag, "k_cache", kc)
        emit(tag, "v_cache", vc)
    elif epi == RESID:
        res = torch.randn(m, n, generator=g).to(torch.bfloat16).to(DEV)
        ops.skinny_gemm(x, Ws, pro, epi, res=res, **kw)
        emit(tag, "res", res)
    else:
        emit(tag, "out", ops.skinny_gemm(x, Ws, pro, epi, **kw))
    if pro == NORM_ADD:
        emit(tag, "xout", kw["xout"])
    if ws is not None:
        emit(tag, "split_ws_counters", ws[:256])   # every form re-arms its counters


def main() -> None:
    ws = ops.split_workspace(DEV)
    h8b, htp2, htp8 = (32, 8, 128), (16, 4, 128), (4, 1, 128)
    rows = [
        # the plan table of csrc/tests/host_check.cpp: decode, shards, serving batches
        (False, 3, 6144, 4096, NORM, ROPE, 2, ws, h8b),
        (False, 3, 4096, 4096, PLAIN, RESID, 2, ws, None),
        (False, 3, 14336, 4096, NORM, SWIGLU, 3, ws, None),
        (False, 3, 14336, 4096, NORM, SWIGLU, 2, ws, None),
        (False, 3, 4096, 14336, PLAIN, RESID, 3, ws, None),
        (False, 3, 128256, 4096, NORM, STORE, 2, ws, None),
        (False, 3, 3072, 4096, NORM, ROPE, 2, ws, htp2),
        (False, 3, 768, 4096, NORM, ROPE, 2, ws, htp8),
        (False, 3, 768, 4096, NORM, ROPE, 0, ws, htp8),
        (False, 3, 1792, 4096, NORM, SWIGLU, 2, ws, None),
        (False, 8, 4096, 4096, PLAIN, RESID, 2, ws, None),
        (False, 16, 6144, 4096, NORM, ROPE, 2, ws, h8b),
        (False, 16, 14336, 4096, NORM, SWIGLU, 3, ws, None),
        (False, 16, 4096, 4096, PLAIN, RESID, 2, ws, None),
        (False, 16, 4096, 4096, PLAIN, RESID, 2, None, None),
        (False, 20, 6144, 4096, NORM, ROPE, 2, ws, h8b),
        (False, 20, 14336, 4096, NORM, SWIGLU, 3, ws, None),
        (False, 20, 4096, 4096, PLAIN, RESID, 2, ws, None),
        (True, 3, 6144, 4096, NORM, ROPE, 0, None, h8b),
        (True, 3, 4096, 14336, NORM, RESID, 0, None, None),
        # the smallest shape of each form
        (False, 3, 48, 96, PLAIN, STORE, 3, None, None),
        (False, 3, 48, 96, NORM_ADD, STORE, 3, None, None),
        (False, 3, 80, 1024, NORM, STORE, 3, ws, None),
        (False, 3, 80, 1024, NORM_ADD, STORE, 3, ws, None),
        (False, 3, 257 * 16, 2048, PLAIN, STORE, 3, ws, None),
        (False, 3, 257 * 16, 2048, NORM, SWIGLU, 3, ws, None),
        (False, 12, 4112, 4096, PLAIN, RESID, 3, ws, None),
        (False, 20, 4112, 4096, NORM, RESID, 3, ws, None),
        (True, 3, 256, 512, PLAIN, STORE, 0, None, None),
        (True, 16, 256, 512, NORM, RESID, 0, None, None),
        (True, 3, 256, 512, NORM, SWIGLU, 0, None, None),
        (True, 3, 256, 512, NORM, ROPE, 0, None, (2, 1, 64)),
        (True, 20, 256, 512, PLAIN, STORE, 0, None, None),   # two launches of <= 16 rows
    ]
    for r in rows:
        run(*r)
        if r[2] * r[3] > 1 << 28:   # drop the lm_head weight at once
            _weights.clear()
    torch.cuda.synchronize()
    print("done", flush=True)


if __name__ == "__main__":
    main()
