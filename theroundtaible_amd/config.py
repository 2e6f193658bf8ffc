"""`.roundtable/config.json` loading, validation and generation.

Parity: `src/utils/config.ts:13-86` (load + validate, same error messages) and
`src/commands/init.ts:138-220` (generated defaults). The schema is accepted
unchanged; unknown fields are tolerated.

MI355X extension: every ``adapter_config[<adapter id>]`` may carry an ``engine``
object that tells the local engine how to host that knight, and a top-level
``engine`` object holds defaults::

    "engine": {"default_model": "llama3-8b", "dtype": "bf16", "weights": "random:0",
               "kv_block_size": 32, "max_new_tokens": 512, "temperature": 0.7,
               "top_p": 0.95, "top_k": 0, "seed": 0, "stop_on_consensus": true,
               "repetition_penalty": 1.0, "repeat_last_n": 64, "presence_penalty": 0.0,
               "frequency_penalty": 0.0, "logit_bias": null},
    "adapter_config": {"claude-cli": {"command": "claude", "args": [],
                                      "engine": {"model": "llama3-8b", "gpus": [0], "tp": 1}}}

Vendor fields (``command``, ``args``, ``env_key``, vendor ``model`` names) are
ignored: no subprocess or HTTPS call is ever made.
"""
from __future__ import annotations

import json
import os
from typing import Any, Dict, List, Optional

from .errors import ConfigError
from .types import RoundtableConfig, dumps_js
from .utils.atomic import read_text

DEFAULT_CAPABILITIES = {
    "Claude": ["architecture", "refactoring", "logic", "debugging", "testing"],
    "Gemini": ["docs", "ui-ux", "summarization", "review", "planning"],
    "GPT": ["communication", "content", "explanation"],
}

ENGINE_DEFAULTS: Dict[str, Any] = {
    "default_model": "llama3-8b",
    "dtype": "bf16",
    "weights": "random:0",
    "kv_block_size": 32,
    "max_new_tokens": 512,
    "temperature": 0.7,
    "top_p": 0.95,
    "top_k": 0,
    "seed": 0,
    "stop_on_consensus": True,
    "ignore_eos": False,
    "kv_cache_fraction": 0.85,
    # logit processors (engine/sampler.py), neutral: logit_bias is {"<token id>": bias} or null
    "repetition_penalty": 1.0,
    "repeat_last_n": 64,
    "presence_penalty": 0.0,
    "frequency_penalty": 0.0,
    "logit_bias": None,
    # every turn whose reply goes to parse_consensus gets a grammar: free text, then a fenced JSON block that
    # obeys the consensus schema, always inside max_new_tokens (consensus.consensus_grammar)
    "consensus_grammar": False,
}


def config_path(project_root: str) -> str:
    return os.path.join(project_root, ".roundtable", "config.json")


def load_config(project_root: str) -> RoundtableConfig:
    p = config_path(project_root)
    if not os.path.exists(p):
        raise ConfigError("No .roundtable/config.json found.", hint='Run "roundtable init" first.')
    try:
        raw = json.loads(read_text(p))
    except ValueError:
        raise ConfigError("Invalid config.json — could not parse JSON.",
                          hint="Check for syntax errors in .roundtable/config.json")
    validate_config(raw)
    return RoundtableConfig.from_dict(raw)


def _is_num(v: Any) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def validate_config(cfg: Dict[str, Any]) -> None:
    if not isinstance(cfg, dict):
        raise ConfigError("config.json must be a JSON object.")
    if not cfg.get("version"):
        raise ConfigError("config.json missing 'version' field.")
    knights = cfg.get("knights")
    if not isinstance(knights, list) or not knights:
        raise ConfigError("config.json must have at least one knight.")
    for k in knights:
        if not isinstance(k, dict) or not k.get("name") or not k.get("adapter"):
            raise ConfigError(f"Knight missing required fields (name, adapter): {json.dumps(k)}")
        if not isinstance(k.get("capabilities"), list):
            raise ConfigError(f'Knight "{k["name"]}" missing capabilities array.')
        if not _is_num(k.get("priority")):
            raise ConfigError(f'Knight "{k["name"]}" missing numeric priority.')
    rules = cfg.get("rules")
    if not rules:
        raise ConfigError("config.json missing 'rules' section.")
    if not _is_num(rules.get("max_rounds")) or rules["max_rounds"] < 1:
        raise ConfigError("rules.max_rounds must be a positive number.")
    ct = rules.get("consensus_threshold")
    if not _is_num(ct) or ct < 0 or ct > 10:
        raise ConfigError("rules.consensus_threshold must be between 0 and 10.")
    tpt = rules.get("timeout_per_turn_seconds")
    if not _is_num(tpt) or tpt < 1:
        raise ConfigError("rules.timeout_per_turn_seconds must be a positive number.")
    if rules.get("round_mode", "sequential") not in ("sequential", "parallel"):
        raise ConfigError("rules.round_mode must be 'sequential' or 'parallel'.")
    if rules.get("prompt_layout", "reference") not in ("reference", "append", "shared"):
        raise ConfigError("rules.prompt_layout must be 'reference', 'append' or 'shared'.")
    if rules.get("placeholder_semantics", "literal") not in ("literal", "reference"):
        raise ConfigError("rules.placeholder_semantics must be 'literal' or 'reference'.")
    if not cfg.get("adapter_config") and cfg.get("adapter_config") != {}:
        raise ConfigError("config.json missing 'adapter_config' section.")
    if cfg.get("adapter_config") is None:
        raise ConfigError("config.json missing 'adapter_config' section.")


WEIGHT_QUANTS = ("none", "fp8", "mxfp4")


def resolve_weight_quant(value: Optional[str]) -> str:
    """A stated ``weight_quant`` ("none" | "fp8" | "mxfp4"), or — when a config says nothing (None / "") —
    the ROUNDTABLE_WEIGHT_QUANT default, else "none"."""
    q = str(value if value else os.environ.get("ROUNDTABLE_WEIGHT_QUANT") or "none").lower()
    if q not in WEIGHT_QUANTS:
        raise ConfigError(f"unknown weight_quant {q!r}", hint=f"One of: {', '.join(WEIGHT_QUANTS)}.")
    return q


KV_DTYPES = ("bf16", "fp8")


def resolve_kv_dtype(value: Optional[str]) -> str:
    """A stated ``kv_dtype`` ("bf16" | "fp8"), or — when a config says nothing (None / "") — the
    ROUNDTABLE_KV_DTYPE default, else "bf16". "fp8": K/V pages hold OCP e4m3fn codes, one byte per
    element, with one fp32 k_scale and v_scale per layer (``kv_scale``)."""
    q = str(value if value else os.environ.get("ROUNDTABLE_KV_DTYPE") or "bf16").lower()
    if q == "bfloat16":
        q = "bf16"
    if q not in KV_DTYPES:
        raise ConfigError(f"unknown kv_dtype {q!r}", hint=f"One of: {', '.join(KV_DTYPES)}.")
    return q


def per_layer_kv_scales(value, n_layers: int, which: str = "k") -> list:
    """One KV scale per layer from one float or a list with one float per layer. The ONE Python copy of
    the scale rule (the launchers repeat it in front of their kernels): every scale a finite number > 0
    whose fp32 value and reciprocal are finite and normal; ConfigError naming kv_dtype otherwise."""
    import math
    vals = list(value) if isinstance(value, (list, tuple)) else [value] * n_layers
    if len(vals) != n_layers:
        raise ConfigError(f"kv_dtype: kv_scale.{which} has {len(vals)} values for {n_layers} layers",
                          hint="One float, or a list with one float per layer.")
    for s in vals:
        if isinstance(s, bool) or not isinstance(s, (int, float)) or not math.isfinite(s) or s <= 0 \
                or float(s) > 3.0e38 or float(s) < 1.2e-38:
            raise ConfigError(f"kv_dtype: kv_scale.{which} must be finite and > 0 (got {s!r})")
    return [float(s) for s in vals]


def resolve_kv_scale(value, n_layers: Optional[int] = None) -> Dict[str, Any]:
    """``kv_scale`` as ``{"k": x, "v": y}``, each one float or a list with one float per layer
    (default 1.0), checked by :func:`per_layer_kv_scales` (``n_layers`` None: a list of any length)."""
    if value is None:
        value = {}
    if not isinstance(value, dict) or set(value) - {"k", "v"}:
        raise ConfigError("kv_dtype: kv_scale must be an object {\"k\": x, \"v\": y}",
                          hint="Each of k / v is one float or a list with one float per layer.")
    out = {}
    for which in ("k", "v"):
        x = value.get(which, 1.0)
        is_list = isinstance(x, (list, tuple))
        vals = per_layer_kv_scales(x, (len(x) if n_layers is None else n_layers) if is_list else 1, which)
        out[which] = vals if is_list else vals[0]
    return out


def engine_settings(config: RoundtableConfig, adapter_id: str) -> Dict[str, Any]:
    """Effective engine settings for one adapter id: defaults <- config.engine <- adapter engine.
    ``weight_quant`` (engine-wide or per knight) comes back resolved: "none" | "fp8" | "mxfp4".
    ``kv_dtype`` (engine-wide or per knight) comes back resolved: "bf16" | "fp8", ``kv_scale`` checked.
    ``consensus_grammar`` (engine-wide or per knight) is a bool; with ``scripted_consensus`` a ConfigError."""
    out = dict(ENGINE_DEFAULTS)
    top = config.raw.get("engine") if isinstance(config.raw, dict) else None
    if isinstance(top, dict):
        out.update(top)
    ac = config.adapter_config.get(adapter_id) or {}
    eng = ac.get("engine") if isinstance(ac, dict) else None
    if isinstance(eng, dict):
        out.update(eng)
    if "model" not in out or not out.get("model"):
        out["model"] = resolve_model_name(ac.get("model") if isinstance(ac, dict) else None,
                                          out["default_model"])
    out["weight_quant"] = resolve_weight_quant(out.get("weight_quant"))
    out["kv_dtype"] = resolve_kv_dtype(out.get("kv_dtype"))
    # kv_scale is read (and checked) only with an fp8 cache: a stray one beside bf16 pages is passed on as is
    if out["kv_dtype"] == "fp8":
        out["kv_scale"] = resolve_kv_scale(out.get("kv_scale"))
    else:
        out["kv_scale"] = out.get("kv_scale") or {}
    if not isinstance(out.get("consensus_grammar", False), bool):
        raise ConfigError(f"{adapter_id}: engine.consensus_grammar must be true or false")
    if out.get("consensus_grammar") and out.get("scripted_consensus"):
        raise ConfigError(f"{adapter_id}: engine.consensus_grammar cannot be combined with engine.scripted_consensus",
                          hint="The script forces the block's tokens; the grammar lets the model write it. Pick one.")
    return out


def processor_settings(st: Dict[str, Any]) -> Dict[str, Any]:
    """The logit-processor keys of an engine settings block as SamplingParams arguments (JSON
    writes ``logit_bias`` token ids as strings); ConfigError for a value outside their ranges."""
    from .engine.sampler import SamplingParams
    bias = st.get("logit_bias")
    try:
        if bias is not None and not isinstance(bias, dict):
            raise ValueError("logit_bias must be an object of token id -> bias")
        out = {"repetition_penalty": float(st.get("repetition_penalty", 1.0)),
               "repeat_last_n": int(st.get("repeat_last_n", 64)),
               "presence_penalty": float(st.get("presence_penalty", 0.0)),
               "frequency_penalty": float(st.get("frequency_penalty", 0.0)),
               "logit_bias": {int(k): float(v) for k, v in bias.items()} if bias else None}
        SamplingParams(**out).check_processors()
    except (TypeError, ValueError) as e:
        raise ConfigError(f"engine sampling settings: {e}",
                          hint="penalties in [-2, 2], repetition_penalty > 0, at most 300 biases in [-100, 100].")
    return out


_MODEL_ALIASES = {
    "llama3-8b": ("llama-3-8b", "llama3-8b", "llama-3.1-8b", "meta-llama-3-8b"),
    "llama3-70b": ("llama-3-70b", "llama3-70b", "llama-3.1-70b", "meta-llama-3-70b"),
    "mistral-7b": ("mistral-7b", "mistral-7b-instruct"),
    # (substring match: "qwen3-14b" does not contain "qwen3-4b", nor does any other pair here overlap)
    "qwen3-0.6b": ("qwen3-0.6b", "qwen-3-0.6b"),
    "qwen3-1.7b": ("qwen3-1.7b", "qwen-3-1.7b"),
    "qwen3-4b": ("qwen3-4b", "qwen-3-4b"),
    "qwen3-8b": ("qwen3-8b", "qwen-3-8b"),
    "qwen3-14b": ("qwen3-14b", "qwen-3-14b"),
    "qwen3-32b": ("qwen3-32b", "qwen-3-32b"),
    "gpt2-small": ("gpt2", "gpt-2", "gpt2-small"),
    "tiny-llama": ("tiny-llama", "tiny"),
}


def resolve_model_name(name: Optional[str], default: str) -> str:
    """Map an ``adapter_config.model`` string onto an engine preset (vendor names -> default)."""
    if not name:
        return default
    low = str(name).lower()
    for preset, aliases in _MODEL_ALIASES.items():
        if any(a in low for a in aliases):
            return preset
    return default


def generate_config(project: str, language: str, knights: List[Dict[str, Any]],
                    engine: Optional[Dict[str, Any]] = None,
                    adapter_engine: Optional[Dict[str, Dict[str, Any]]] = None) -> Dict[str, Any]:
    """Build a config dict in the reference's shape (init.ts:138-220) + engine extensions.

    ``knights`` items: ``{"name", "adapter", "fallback"?, "capabilities"?}``.
    """
    out_knights = []
    for i, k in enumerate(knights, start=1):
        d = {"name": k["name"], "adapter": k["adapter"],
             "capabilities": k.get("capabilities") or DEFAULT_CAPABILITIES.get(k["name"], ["general"]),
             "priority": i}
        if k.get("fallback"):
            d["fallback"] = k["fallback"]
        out_knights.append(d)
    adapter_config: Dict[str, Any] = {
        "claude-cli": {"command": "claude", "args": ["-p", "{prompt}", "--print"]},
        "claude-api": {"model": "claude-sonnet-4-6", "env_key": "ANTHROPIC_API_KEY"},
        "gemini-cli": {"command": "gemini", "args": ["-p", "{prompt}"], "model": "gemini-2.5-pro"},
        "gemini-api": {"model": "gemini-2.5-flash", "env_key": "GEMINI_API_KEY"},
        "openai-cli": {"command": "codex", "args": ["exec", "{prompt}"]},
        "openai-api": {"model": "gpt-5.2", "env_key": "OPENAI_API_KEY"},
    }
    for aid, eng in (adapter_engine or {}).items():
        adapter_config.setdefault(aid, {})["engine"] = eng
    cfg = {
        "version": "1.0", "project": project, "language": language, "knights": out_knights,
        "rules": {"max_rounds": 5, "consensus_threshold": 9, "timeout_per_turn_seconds": 120,
                  "escalate_to_user_after": 3, "auto_execute": False,
                  "ignore": [".git", "node_modules", "dist", "build", ".next"],
                  "round_mode": "sequential", "prompt_layout": "reference"},
        "chronicle": ".roundtable/chronicle.md",
        "adapter_config": adapter_config,
    }
    if engine:
        cfg["engine"] = engine
    return cfg


def write_config(project_root: str, cfg: Dict[str, Any]) -> None:
    from .utils.atomic import atomic_write_text
    atomic_write_text(config_path(project_root), dumps_js(cfg))
