"""Probe: what the two logprob launches (csrc/logprobs.hip) cost inside a captured step, next to the
K6 sampler launch they follow.

B = 3 rows, V = 128256, bf16 logits (the bench's batch and Llama-3's vocabulary), every row asking
for n_top = 0 / 5 / 20, plus the launch pair with every row off (n_top = -1: what a neutral row of a
logprobs graph pays). Per configuration three hipGraphs of REP back-to-back iterations are timed with
device events over REPLAYS replays (L2-hot, as in the decode step, where the lm_head GEMM has just
written the logits and K6 has just read them):

* ``lp``        REP x {logprob_chunks, logprob_merge}
* ``smp``       REP x smp_kernel (temperature 0.7, top-p 0.95) — the yardstick, same run
* ``smp+lp``    REP x {smp_kernel, logprob_chunks, logprob_merge}; ``smp+lp - smp`` is the marginal
                cost in place

The logprob kernels only read the logits, so the sampler's input is the same in every iteration.
The ``ids`` form is timed (record row 0); the graph form differs by one load of the step counter.

    python tools/probes/logprobs.py --out table.md
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
    g = torch.Generator().manual_seed(9)
    logits = (3.0 * torch.randn(B, V, generator=g)).to(torch.bfloat16).to(DEV)
    temp = torch.full((B,), 0.7, device=DEV)
    top_p = torch.full((B,), 0.95, device=DEV)
    top_k = torch.zeros(B, dtype=torch.int32, device=DEV)
    seeds = torch.arange(B, dtype=torch.int64, device=DEV)
    offs = torch.full((B,), 7, dtype=torch.int64, device=DEV)
    nxt = torch.zeros(B, dtype=torch.int64, device=DEV)
    ws = ops.sample_workspace(B, DEV)
    lp = ops.LogProbs(B, DEV, 1)

    def smp():
        ops.sample(logits, temp, top_p, top_k, seeds, offs, out=nxt, ws=ws)

    def logp():
        ops.token_logprobs(logits, lp, ids=nxt)

    def both():
        smp()
        logp()

    rows = []
    for n_top in (0, 5, 20, -1):
        lp.n_top.fill_(n_top)
        r = {"n_top": n_top, "lp_us": time_graph(logp), "smp_us": time_graph(smp), "both_us": time_graph(both)}
        r["marginal_us"] = r["both_us"] - r["smp_us"]
        print(json.dumps(r), flush=True)
        rows.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("| n_top (every row) | logprob launches µs | smp_kernel µs | smp + logprobs µs | marginal µs |\n"
                    "|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['n_top'] if r['n_top'] >= 0 else 'off (-1)'} | {r['lp_us']:.2f} | {r['smp_us']:.2f} | "
                        f"{r['both_us']:.2f} | {r['marginal_us']:.2f} |\n")
            f.write(f"\n{torch.cuda.get_device_name(0)}; B = {B}, V = {V}, bf16; {REP} iterations per graph, "
                    f"{REPLAYS} replays per window, best of 3 windows.\n")


if __name__ == "__main__":
    main()
