"""Section-6 measurements: the QK-norm kernel per call, and qkv EPI_STORE + K2n against the fused ROPE epilogue.
Each variant is a captured graph of REP back-to-back calls over ROT distinct weight copies (ROT x 50 MB > the 256 MiB
Infinity Cache for bf16, so weights stream from HBM as in a decode step); variants alternate, 7 rounds, median."""
import json
import statistics
import sys

import torch

from theroundtaible_amd import ops
from theroundtaible_amd.ops import reference as ref

DEV = "cuda"
BF = torch.bfloat16
HQ, HKV, D, K = 32, 8, 128, 4096
N = (HQ + 2 * HKV) * D
EPS = 1e-6
ROUNDS = 7


def graph_of(fn, rep):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(3):
            fn(0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for i in range(rep):
                fn(i)
    torch.cuda.synchronize()
    return g


def time_graph(g, rep, n=5):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g.replay()
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / (n * rep)      # us per call


def alternate(variants, rep):
    graphs = {k: graph_of(f, rep) for k, f in variants.items()}
    t = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            t[k].append(time_graph(g, rep))
    return {k: {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3)}
            for k, v in t.items()}


def operands(B, kv8):
    g = torch.Generator(device=DEV).manual_seed(B)
    nb = 64
    pos = torch.randint(0, 4000, (B,), device=DEV, dtype=torch.int64, generator=g)
    slots = torch.randperm(nb * 32, device=DEV, generator=g)[:B].to(torch.int64)
    dt = torch.uint8 if kv8 else BF
    kc = torch.zeros(nb, HKV, 32, D, dtype=dt, device=DEV)
    vc = torch.zeros(nb, HKV, D, 32, dtype=dt, device=DEV)
    return pos, slots, kc, vc


def main(out):
    res = {"shape": {"Hq": HQ, "Hkv": HKV, "D": D, "K": K, "N": N}, "kernel": {}, "qkv": {}}
    cs = ref.rope_cos_sin(8192, D, 1e6, DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    gq = (1 + 0.3 * torch.randn(D, device=DEV, generator=g)).to(BF)
    gk = (1 + 0.3 * torch.randn(D, device=DEV, generator=g)).to(BF)
    # (a) the kernel alone
    for B in (3, 16):
        qkv = torch.randn(B, N, device=DEV, generator=g).to(BF)
        var = {}
        for kv8 in (False, True):
            pos, slots, kc, vc = operands(B, kv8)
            var["fp8" if kv8 else "bf16"] = (lambda i, pos=pos, slots=slots, kc=kc, vc=vc: ops.qk_norm_rope_and_cache(
                qkv, gq, gk, EPS, pos, cs, kc, vc, slots, HQ, HKV, D, 0.5, 0.5))
        pos, slots, kc, vc = operands(B, False)
        var["rope_cache_kernel bf16 (K2, no norm)"] = (lambda i, pos=pos, slots=slots, kc=kc, vc=vc: ops.rope_and_cache(
            qkv, pos, cs, kc, vc, slots, HQ, HKV, D))
        res["kernel"][f"B={B}"] = alternate(var, 200)
        print("kernel", B, res["kernel"][f"B={B}"], flush=True)
    # (b) qkv GEMM: EPI_STORE + K2n vs the fused ROPE epilogue, per weight type
    ROT = 8
    gamma = (1 + 0.1 * torch.randn(K, device=DEV, generator=g)).to(BF)
    sw = ops.split_workspace(torch.device(DEV))
    for wt in ("bf16", "fp8", "mxfp4"):
        shuf = {"bf16": lambda W, **kw: (ops.shuffle_weight(W, gamma, **kw), None),
                "fp8": lambda W, **kw: ops.shuffle_weight_fp8(W, gamma, **kw),
                "mxfp4": lambda W, **kw: ops.shuffle_weight_mxfp4(W, gamma, **kw)}[wt]
        plain, roped = [], []
        for r in range(ROT):
            W = (0.02 * torch.randn(N, K, device=DEV, generator=g)).to(BF)
            plain.append(shuf(W))
            roped.append(shuf(W, rope_heads=HQ + HKV, head_dim=D))
            del W
        kw = {} if wt != "bf16" else dict(split_ws=sw, split_mode=ops.SPLIT_K)
        for B in (3, 16):
            x = torch.randn(B, K, device=DEV, generator=g).to(BF)
            pos, slots, kc, vc = operands(B, False)

            def fused(i):
                Ws, sc = roped[i % ROT]
                return ops.skinny_gemm_rope(x, Ws, ops.PRO_NORM, pos, cs, kc, vc, slots, HQ, HKV, D, EPS, wscale=sc, **kw)

            def store_only(i):
                Ws, sc = plain[i % ROT]
                return ops.skinny_gemm(x, Ws, ops.PRO_NORM, ops.EPI_STORE, eps=EPS, wscale=sc, **kw)

            def store_then_k2n(i):
                qkv = store_only(i)
                return ops.qk_norm_rope_and_cache(qkv, gq, gk, EPS, pos, cs, kc, vc, slots, HQ, HKV, D)

            r = alternate({"fused_rope_epilogue": fused, "epi_store": store_only, "epi_store+k2n": store_then_k2n}, 48)
            r["extra_us"] = round(r["epi_store+k2n"]["median_us"] - r["fused_rope_epilogue"]["median_us"], 3)
            res["qkv"][f"{wt} B={B}"] = r
            print("qkv", wt, B, r, flush=True)
        del plain, roped
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
