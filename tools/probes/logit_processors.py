"""Probe: what the logit-processor launch (csrc/logit_proc.hip) costs inside a captured step, next
to the K6 sampler launch it precedes.

B = 3 rows, V = 128256, bf16 logits (the bench's batch and Llama-3's vocabulary), every row active
(repetition over the whole window, frequency and presence over the reply), host histories of
0 / 64 / 512 / 2048 random tokens, each with and without 300 biases. Per configuration three
hipGraphs of REP back-to-back launches are timed with device events over REPLAYS replays (L2-hot,
as in the decode step, where the lm_head GEMM has just written the logits):

* ``proc``       REP x logit_proc_kernel
* ``smp``        REP x smp_kernel (temperature 0.7, top-p 0.95) — the yardstick, same run
* ``proc+smp``   REP x {logit_proc_kernel, smp_kernel}; ``proc+smp - smp`` is the marginal cost in place

The parameters are chosen so that a bf16 logit of ordinary size keeps its value under them (rp =
1.0001, fp = pp = 1e-6, biases of +-1e-3 round away once |l| reaches about 1), so thousands of
in-place applications leave the sampler's input nearly as it was (``max_drift`` reports the largest
change); the kernel's work does not depend on the values.

    python tools/probes/logit_processors.py --out table.md
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from theroundtaible_amd import ops  # noqa: E402

DEV = "cuda"
B, V = 3, 128256
REP, REPLAYS, WARM = 20, 50, 5


def make_proc(n_hist: int, n_bias: int, g: torch.Generator) -> "ops.LogitProc":
    p = ops.LogitProc(B, "cpu")
    p.hist[:, :n_hist] = torch.randint(0, V, (B, n_hist), generator=g).to(torch.int32)
    p.hist_len.fill_(n_hist)
    p.reply_from.fill_(0)
    p.rp.fill_(1.0001)
    p.last_n.fill_(-1)
    p.fp.fill_(1e-6)
    p.pp.fill_(1e-6)
    if n_bias:
        p.bias_tok[:, :n_bias] = torch.stack([torch.randperm(V, generator=g)[:n_bias] for _ in range(B)]).to(torch.int32)
        p.bias_val[:, :n_bias] = 1e-3 * (2.0 * torch.randint(0, 2, (B, n_bias), generator=g) - 1.0)
        p.bias_n.fill_(n_bias)
    d = ops.LogitProc(B, DEV)
    for f in ("hist", "hist_len", "reply_from", "rp", "last_n", "pp", "fp", "bias_tok", "bias_val", "bias_n"):
        getattr(d, f).copy_(getattr(p, f))
    return d


def time_graph(body) -> float:
    """µs per iteration of ``body`` (captured REP times, replayed REPLAYS times)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REP):
            body()
    for _ in range(WARM):
        g.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):                                   # three windows; the quietest one
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPLAYS):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / (REPLAYS * REP))
    return best


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the markdown table here")
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.native_available(), "needs the GPU and the built extension"
    g = torch.Generator().manual_seed(8)
    logits0 = (3.0 * torch.randn(B, V, generator=g)).to(torch.bfloat16).to(DEV)
    logits = logits0.clone()
    temp = torch.full((B,), 0.7, device=DEV)
    top_p = torch.full((B,), 0.95, device=DEV)
    top_k = torch.zeros(B, dtype=torch.int32, device=DEV)
    seeds = torch.arange(B, dtype=torch.int64, device=DEV)
    offs = torch.full((B,), 7, dtype=torch.int64, device=DEV)
    nxt = torch.zeros(B, dtype=torch.int64, device=DEV)
    ws = ops.sample_workspace(B, DEV)
    out = torch.zeros(64, B, dtype=torch.int64, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)

    def smp():
        ops.sample(logits, temp, top_p, top_k, seeds, offs, out=nxt, ws=ws)

    rows = []
    for n_hist in (0, 64, 512, 2048):
        for n_bias in (0, 300):
            proc = make_proc(n_hist, n_bias, g)

            def lp():
                ops.apply_logit_processors(logits, proc, out, step)

            def both():
                lp()
                smp()
            logits.copy_(logits0)
            r = {"hist": n_hist, "biases": n_bias, "proc_us": time_graph(lp), "smp_us": time_graph(smp),
                 "both_us": time_graph(both)}
            r["marginal_us"] = r["both_us"] - r["smp_us"]
            r["max_drift"] = float((logits.float() - logits0.float()).abs().max())
            print(json.dumps(r), flush=True)
            rows.append(r)
    neutral = ops.LogitProc(B, DEV)
    rows.append({"hist": "neutral rows", "biases": 0, "smp_us": time_graph(smp),
                 "proc_us": time_graph(lambda: ops.apply_logit_processors(logits, neutral, out, step))})
    print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("| history tokens | biases | logit_proc µs | smp_kernel µs | both µs | both - smp µs |\n"
                    "|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['hist']} | {r['biases']} | {r['proc_us']:.2f} | {r['smp_us']:.2f} | "
                        + (f"{r['both_us']:.2f} | {r['marginal_us']:.2f} |\n" if "both_us" in r else "- | - |\n"))
            f.write(f"\n{torch.cuda.get_device_name(0)}; B = {B}, V = {V}, bf16; {REP} launches per graph, "
                    f"{REPLAYS} replays per window, best of 3 windows.\n")


if __name__ == "__main__":
    main()
