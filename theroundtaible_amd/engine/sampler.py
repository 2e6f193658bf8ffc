"""Sampling parameters (K6 does the work: csrc/sampling.hip)."""
from __future__ import annotations

import hashlib
from typing import Dict, Optional
from dataclasses import dataclass

MAX_LOGIT_BIAS = 300     # OpenAI's limit; ops.LOGIT_PROC_MAX_BIAS
MAX_TOP_LOGPROBS = 20    # OpenAI's limit; ops.MAX_TOP_LOGPROBS


@dataclass
class SamplingParams:
    temperature: float = 0.7
    top_p: float = 0.95
    top_k: int = 0
    seed: int = 0
    max_new_tokens: int = 512
    ignore_eos: bool = False
    stop_on_consensus: bool = True
    # teacher-forced text appended after the sampled tokens (knights/script.py scripted consensus)
    forced_tail: Optional[str] = None
    # logit processors (csrc/logit_proc.hip), applied before temperature / top-k / top-p; all neutral
    # by default. Order: logit_bias, repetition penalty, then frequency and presence.
    repetition_penalty: float = 1.0     # HF / Ollama form over the last ``repeat_last_n`` tokens, prompt included
    repeat_last_n: int = 64             # 0 = off, -1 = the cap (ops.LOGIT_PROC_WINDOW)
    presence_penalty: float = 0.0       # OpenAI form, over the tokens of this reply
    frequency_penalty: float = 0.0      # OpenAI form, times the token's count in this reply
    logit_bias: Optional[Dict[int, float]] = None   # {token id: bias}, at most 300 entries in [-100, 100]
    # logprobs (csrc/logprobs.hip): None = off; n in 0..20 = every sampled token's log-probability plus
    # the n most likely alternatives, on the logits as sampled from (after the processors above,
    # before temperature / top-k / top-p). Never changes the sampled ids.
    logprobs: Optional[int] = None
    # grammar-constrained decoding (engine/grammar.py, csrc/grammar_mask.hip): None = off, or
    # {"type": "json_object"} | {"type": "json_schema", "schema": {...}} | {"type": "regex", "pattern": "..."}.
    # Tokens the grammar cannot accept next get -inf after the processors above and before sampling;
    # the reply ends with a stop id once the grammar accepts (or is cut short by max_new_tokens).
    # Also {"type": "tail", "open": "...", "body": <json_schema or regex spec>, "close": "..."}: free text up to
    # the first ``open``, then the body, then ``close`` (a grammar that switches on mid-reply).
    grammar: Optional[dict] = None
    # with a grammar: the reply's ids end with a stop id after at most max_new_tokens tokens and the text
    # before it is accepted by the grammar (csrc/grammar_budget.hip masks by the tokens left as well).
    # max_new_tokens below the grammar's minimum is a ValueError before prefill.
    grammar_finish: bool = False
    # set by the engine when max_new_tokens is a decode chunk's, not the reply's: the reply's whole budget
    grammar_budget: Optional[int] = None

    def wants_grammar(self) -> bool:
        return self.grammar is not None

    def wants_grammar_budget(self) -> bool:
        """The row needs the budgeted mask launch: ``grammar_finish``, or a ``tail`` grammar (its free phase
        is that launch's shortcut)."""
        return self.grammar is not None and (self.grammar_finish or (isinstance(self.grammar, dict)
                                                                      and self.grammar.get("type") == "tail"))

    def reply_budget(self) -> Optional[int]:
        """Tokens the whole reply may hold under ``grammar_finish``; None when nothing bounds the grammar."""
        if self.grammar is None or not self.grammar_finish:
            return None
        return int(self.grammar_budget if self.grammar_budget is not None else max(1, self.max_new_tokens))

    def check_grammar(self) -> None:
        """ValueError for a spec the compiler refuses and for ``ignore_eos`` with a grammar: a
        constrained reply ends with a stop id (serve.py answers 400)."""
        if self.grammar is None:
            if self.grammar_finish:
                raise ValueError("grammar_finish needs a grammar")
            return
        from .grammar import compile_grammar
        compile_grammar(self.grammar)
        if self.ignore_eos:
            raise ValueError("ignore_eos cannot be combined with a grammar: a constrained reply ends with a stop id")

    def wants_logprobs(self) -> bool:
        return self.logprobs is not None

    def check_logprobs(self) -> None:
        """ValueError for a ``logprobs`` outside 0..20 (serve.py answers 400)."""
        n = self.logprobs
        if n is None:
            return
        if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= MAX_TOP_LOGPROBS:
            raise ValueError(f"logprobs must be an integer in 0..{MAX_TOP_LOGPROBS}, got {n!r}")

    def has_processors(self) -> bool:
        """False when every processor field is neutral: such a row is sampled exactly as before."""
        return bool((self.repetition_penalty != 1.0 and self.repeat_last_n != 0) or self.presence_penalty != 0.0
                    or self.frequency_penalty != 0.0 or self.logit_bias)

    def check_processors(self, vocab: Optional[int] = None) -> None:
        """ValueError for values the processors do not accept (the limits serve.py answers 400 for)."""
        for name in ("presence_penalty", "frequency_penalty"):
            v = getattr(self, name)
            if not -2.0 <= float(v) <= 2.0:
                raise ValueError(f"{name} must be in [-2, 2], got {v}")
        if not float(self.repetition_penalty) > 0.0:
            raise ValueError(f"repetition_penalty must be > 0, got {self.repetition_penalty}")
        bias = self.logit_bias or {}
        if len(bias) > MAX_LOGIT_BIAS:
            raise ValueError(f"logit_bias has {len(bias)} entries; at most {MAX_LOGIT_BIAS} are allowed")
        for tok, v in bias.items():
            if not -100.0 <= float(v) <= 100.0:
                raise ValueError(f"logit_bias[{tok}] must be in [-100, 100], got {v}")
            if int(tok) < 0 or (vocab is not None and int(tok) >= vocab):
                raise ValueError(f"logit_bias token id {tok} is outside the vocabulary")

    def seq_seed(self, seq_key: str) -> int:
        """Deterministic per (engine seed, knight): sample i of a knight depends only on (seed, knight, position)."""
        h = hashlib.sha256(f"{self.seed}:{seq_key}".encode()).digest()
        return int.from_bytes(h[:8], "little") & ((1 << 63) - 1)
