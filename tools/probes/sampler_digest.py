#!/usr/bin/env python3
"""Token ids of the one-launch sampler for fixed inputs, through the public ``ops`` API only.

    python tools/probes/sampler_digest.py [--sha] > tokens.txt
    RT_SMP_PROBE=5 python tools/probes/sampler_digest.py [--sha] > paths.txt

One line per launch: the case name, the RNG offset and the row's token ids. Two trees whose
sampler draws the same tokens print the same listing line for line; with ``RT_SMP_PROBE=5`` (read
once per process, so a second process) the ids are replaced by the path that decided each row
(csrc/sampling.hip ``PATH_*``), and two trees that decide every row the same way print the same
listing again. Inputs are generated on the CPU with fixed seeds.

``--sha`` prints one line per case in place of its launches: their number, the sha256 of exactly
the lines the full listing would hold and, under ``RT_SMP_PROBE=5``, how many rows each path
decided. That is the form to keep as a record (the full listing is 1200 long lines).

Cases: bf16 and fp32 rows at V = 128256 and 32000, as 16-byte-aligned rows (the vector kernels)
and as a view one element into a wider tensor (the non-vector kernels); peaked, near-flat (x 0.05)
and tie-heavy (rounded) rows; one row per parameter set (``PARAMS``); OFFSETS launches per case
on one persistent workspace, so every launch after the first runs on the grid scale the previous
one adapted. Then ``sample_advance`` chained over a few steps, every state tensor printed.
"""
import collections
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from theroundtaible_amd import ops  # noqa: E402

DEV = "cuda"
OFFSETS = 50
# (temperature, top_p, top_k) of each row of a case
PARAMS = [(0.0, 1.0, 0), (0.8, 1.0, 0), (0.8, 0.3, 0), (0.8, 0.9, 0), (0.7, 0.95, 0), (0.8, 1.0, 5), (0.8, 1.0, 40),
          (0.8, 1.0, 64), (0.8, 1.0, 200), (0.8, 1.0, 1000), (0.8, 0.9, 40), (0.8, 0.7, 200)]
KINDS = {"peaked": lambda x: x * 3.0, "flat": lambda x: x * 0.05, "ties": lambda x: torch.round(x * 2) / 2}
SHA = "--sha" in sys.argv[1:]
PATHS = os.environ.get("RT_SMP_PROBE") == "5"


class Case:
    """The launches of one case: printed as they come, or (--sha) as one line when the case ends."""

    def __init__(self, tag: str):
        self.tag, self.n, self.h, self.paths = tag, 0, hashlib.sha256(), collections.Counter()

    def launch(self, detail: str, toks) -> None:
        line = f"{self.tag} {detail}"
        if not SHA:
            print(line, flush=True)
        self.n += 1
        self.h.update((line + "\n").encode())
        self.paths.update(toks)

    def end(self) -> None:
        if SHA:
            by_path = f" rows_per_path={dict(sorted(self.paths.items()))}" if PATHS else ""
            print(f"{self.tag} launches={self.n} sha256={self.h.hexdigest()}{by_path}", flush=True)


def rows(kind: str, dtype, V: int, aligned: bool, seed: int) -> torch.Tensor:
    B = len(PARAMS)
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = KINDS[kind](torch.randn(B, V, generator=g) * 2.0).to(torch.bfloat16).to(dtype)
    if aligned:
        return x.to(DEV)
    big = torch.zeros(B, V + 9, dtype=dtype)
    big[:, 1:1 + V] = x
    return big.to(DEV)[:, 1:1 + V]


def sample_cases() -> None:
    B = len(PARAMS)
    temp = torch.tensor([p[0] for p in PARAMS], device=DEV)
    top_p = torch.tensor([p[1] for p in PARAMS], device=DEV)
    top_k = torch.tensor([p[2] for p in PARAMS], dtype=torch.int32, device=DEV)
    out = torch.empty(B, dtype=torch.int64, device=DEV)
    seed = 0
    for dtype, dname in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        for V in (128256, 32000):
            for aligned in (True, False):
                for kind in KINDS:
                    seed += 1
                    lg = rows(kind, dtype, V, aligned, 4000 + seed)
                    ws = ops.sample_workspace(B, DEV)
                    seeds = torch.arange(B, dtype=torch.int64, device=DEV) * 104729 + seed
                    case = Case(f"{dname} V={V} {'aligned' if aligned else 'unaligned'} {kind}")
                    for o in range(OFFSETS):
                        offs = torch.arange(B, dtype=torch.int64, device=DEV) + 37 * o
                        ops.sample(lg, temp, top_p, top_k, seeds, offs, out, ws=ws)
                        case.launch(f"offset={o} {out.tolist()}", out.tolist())
                    case.end()


def advance_cases() -> None:
    B, V, H, bs, maxb, steps = 5, 32000, 64, 32, 8, 6
    g = torch.Generator(device="cpu").manual_seed(77)
    embed = torch.randn(V, H, generator=g).to(torch.bfloat16).to(DEV)
    bt = torch.randperm(64, generator=g)[:B * maxb].to(torch.int32).reshape(B, maxb).to(DEV)
    seeds = torch.arange(B, dtype=torch.int64, device=DEV) * 31 + 5
    for mode, (t, p, k) in (("greedy", (0.0, 1.0, 0)), ("top_p", (0.8, 0.9, 0)), ("top_k", (0.8, 1.0, 40)),
                            ("top_k_p", (0.8, 0.8, 200))):
        temp = torch.full((B,), t, device=DEV)
        top_p = torch.full((B,), p, device=DEV)
        top_k = torch.full((B,), k, dtype=torch.int32, device=DEV)
        pos = torch.tensor([3, 40, 77, 100, 31], dtype=torch.int64, device=DEV)   # row 1 crosses a block
        st = dict(out=torch.zeros(4, B, dtype=torch.int64, device=DEV), ids=torch.zeros(B, dtype=torch.int64, device=DEV),
                  pos=pos, ctx=(pos + 1).to(torch.int32), step=torch.zeros(1, dtype=torch.int64, device=DEV),
                  slots=torch.zeros(B, dtype=torch.int64, device=DEV), offs=pos + 1,
                  res=torch.zeros(B, H, dtype=torch.bfloat16, device=DEV))
        ws = ops.sample_workspace(B, DEV)
        nxt = torch.zeros(B, dtype=torch.int64, device=DEV)
        case = Case(f"advance {mode}")
        for step in range(steps):           # more steps than rows of `out`: the record stops, the state goes on
            lg = (torch.randn(B, V, generator=g) * 3.0).to(torch.bfloat16).to(DEV)
            ops.sample_advance(lg, temp, top_p, top_k, seeds, st["offs"], ws, nxt, st["out"], st["ids"], st["pos"],
                               st["ctx"], st["step"], st["slots"], st["res"], bt, embed, bs)
            line = [f"tok={nxt.tolist()}"]
            for name, v in st.items():
                line.append(f"{name}={v.view(torch.int16).tolist() if name == 'res' else v.tolist()}")
            case.launch(f"step={step} " + " ".join(line), nxt.tolist())
        case.end()


def main() -> None:
    sample_cases()
    advance_cases()
    torch.cuda.synchronize()
    print("done", flush=True)


if __name__ == "__main__":
    main()
