#!/usr/bin/env python3
"""Probe: prefill-logit cosine and relative L2 error of the mxfp4-weight engine (and, beside it, the
fp8-weight engine) against the bf16 engine on the same random weights (Llama-3-8B, 2 layers and full
depth). A record, not a pass bound: random weights have no outliers to protect and no trained logit
margins.

    python tools/probes/mxfp4_quality.py
"""
import gc
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from theroundtaible_amd.engine import Engine, EngineConfig  # noqa: E402


def logits(quant, layers):
    kw = dict(model="llama3-8b", weights="random-full:5", device="cuda:0", num_blocks=256, use_graphs=False,
              weight_quant=quant, weight_residency="shuffled")
    if layers:
        kw["model_overrides"] = {"n_layers": layers}
    e = Engine(EngineConfig(**kw))
    ids = e.encode_prompt("De ridders van de ronde tafel bespreken de architectuur van de cache-laag. " * 6)
    out = e.prefill([(e.kv.seq("a"), ids)]).float().cpu()
    res = e.weight_residency
    del e
    gc.collect()
    torch.cuda.empty_cache()
    return out, len(ids), res


for layers in (2, None):
    a, n, ra = logits("none", layers)
    for quant in ("fp8", "mxfp4"):
        b, _, rb = logits(quant, layers)
        cos = torch.nn.functional.cosine_similarity(a, b, dim=-1)
        rel = ((a - b).norm() / a.norm()).item()
        print(f"llama3-8b layers={layers or 32} prompt={n} tokens residency {ra} vs {rb}: last-row prefill logit "
              f"cosine min {cos.min().item():.5f} mean {cos.mean().item():.5f}, relative L2 error {rel:.4f}, "
              f"argmax equal {bool((a.argmax(-1) == b.argmax(-1)).all())}", flush=True)
