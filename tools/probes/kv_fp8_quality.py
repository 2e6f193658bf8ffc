#!/usr/bin/env python3
"""Probe: prefill-logit cosine, relative L2 error and greedy-token agreement of the fp8-KV engine
(kv_dtype "fp8", scales 1.0) against the bf16-KV engine on the same random weights (Llama-3-8B, 2 layers
and full depth). Prefill attention reads the pages the same forward wrote, so the last-row logits already
see quantised K/V. A record, not a pass bound: random weights have no outliers to protect and no trained
logit margins.

    python tools/probes/kv_fp8_quality.py
"""
import gc
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from theroundtaible_amd.engine import Engine, EngineConfig, SamplingParams, Turn  # noqa: E402

PROMPT = "De ridders van de ronde tafel bespreken de architectuur van de cache-laag. " * 6
NEW = 48


def run(kv_dtype, layers):
    kw = dict(model="llama3-8b", weights="random-full:5", device="cuda:0", num_blocks=256, use_graphs=False,
              kv_dtype=kv_dtype, weight_residency="shuffled")
    if layers:
        kw["model_overrides"] = {"n_layers": layers}
    e = Engine(EngineConfig(**kw))
    ids = e.encode_prompt(PROMPT)
    out = e.prefill([(e.kv.seq("a"), ids)]).float().cpu()
    e.release("a")
    sp = SamplingParams(temperature=0.0, max_new_tokens=NEW, ignore_eos=True, stop_on_consensus=False)
    t = e.run_turns([Turn("g", PROMPT, sp)])[0]
    assert t.error is None, t.error
    del e
    gc.collect()
    torch.cuda.empty_cache()
    return out, len(ids), list(t.ids)


for layers in (2, None):
    a, n, ta = run("bf16", layers)
    b, _, tb = run("fp8", layers)
    cos = torch.nn.functional.cosine_similarity(a, b, dim=-1)
    rel = ((a - b).norm() / a.norm()).item()
    same = sum(x == y for x, y in zip(ta, tb))
    first = next((i for i, (x, y) in enumerate(zip(ta, tb)) if x != y), NEW)
    print(f"llama3-8b layers={layers or 32} prompt={n} tokens, fp8 KV vs bf16 KV: last-row prefill logit cosine min "
          f"{cos.min().item():.5f} mean {cos.mean().item():.5f}, relative L2 error {rel:.4f}, argmax equal "
          f"{bool((a.argmax(-1) == b.argmax(-1)).all())}; greedy decode of {NEW} tokens: {same} equal, first "
          f"difference at token {first}", flush=True)
