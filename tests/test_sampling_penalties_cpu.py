"""Token penalties and logit_bias through the engine and the serve front end, on the CPU engine:
bans hold from the first token on, neutral values change nothing, OpenAI and Ollama requests carry
the fields (and get 400 for values outside their ranges), a chunked serve decode counts a reply's
tokens across its chunks, and a tp 2 server gives the tp 1 server's ids under bans."""
import json
import os
import subprocess
import sys
import time
import urllib.error
import urllib.request

import pytest
import torch

from test_distributed_cpu import ROOT, free_port
from theroundtaible_amd.config import ENGINE_DEFAULTS, processor_settings
from theroundtaible_amd.engine import Engine, EngineConfig, SamplingParams, Turn
from theroundtaible_amd.errors import ConfigError
from theroundtaible_amd.serve import build_server

PROMPT = "Hallo tafel, wat is het plan voor vandaag?"


def greedy(n=16, **kw):
    return SamplingParams(temperature=0.0, max_new_tokens=n, ignore_eos=True, stop_on_consensus=False, **kw)


def cpu_engine(**kw):
    cfg = dict(model="tiny-llama", device="cpu", dtype="fp32", num_blocks=128, weights="random:2")
    cfg.update(kw)
    return Engine(EngineConfig(**cfg))


def _post(url, body):
    req = urllib.request.Request(url, data=json.dumps(body).encode(), method="POST",
                                 headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(req, timeout=120) as r:
        return r.status, r.read().decode()


# ---- engine ---------------------------------------------------------------------------------------

def test_defaults_are_neutral():
    p = SamplingParams()
    assert not p.has_processors()
    assert (p.repetition_penalty, p.repeat_last_n, p.presence_penalty, p.frequency_penalty, p.logit_bias) == \
        (1.0, 64, 0.0, 0.0, None)
    assert not SamplingParams(repetition_penalty=1.3, repeat_last_n=0).has_processors()
    assert SamplingParams(logit_bias={1: 0.5}).has_processors()


def test_engine_bans_hold_from_the_first_token_and_neutral_changes_nothing():
    e = cpu_engine()
    base = e.run_turns([Turn("K1", PROMPT, greedy())])[0]
    assert base.error is None and len(base.ids) == 16
    neutral = e.run_turns([Turn("K2", PROMPT, greedy(repetition_penalty=1.0, repeat_last_n=64, presence_penalty=0.0,
                                                      frequency_penalty=0.0, logit_bias=None))])[0]
    assert neutral.ids == base.ids
    banned = e.run_turns([Turn("K3", PROMPT, greedy(logit_bias={a: -100.0 for a in set(base.ids)}))])[0]
    assert banned.error is None and len(banned.ids) == 16
    assert not set(banned.ids) & set(base.ids)
    # a second round of bans on top: the first token obeys them as well
    again = e.run_turns([Turn("K4", PROMPT, greedy(logit_bias={a: -100.0 for a in set(base.ids) | set(banned.ids)}))])[0]
    assert not set(again.ids) & (set(base.ids) | set(banned.ids))


def test_engine_mixed_batch_leaves_the_neutral_row():
    e = cpu_engine()
    base = e.run_turns([Turn("K1", PROMPT, greedy()), Turn("K2", PROMPT + " Anders.", greedy())])
    both = e.run_turns([Turn("K1b", PROMPT, greedy()),
                        Turn("K2b", PROMPT + " Anders.", greedy(logit_bias={base[1].ids[3]: -100.0}))])
    assert both[0].ids == base[0].ids
    assert both[1].ids[:3] == base[1].ids[:3] and base[1].ids[3] not in both[1].ids


def test_dist_greedy_is_off_for_a_batch_with_processors():
    from theroundtaible_amd.parallel.tp import TPInfo
    e = object.__new__(Engine)
    e.tp = TPInfo(size=2, rank=0)
    e.on_gpu = False
    e.ecfg = EngineConfig(device="cpu")
    plain, banned = Turn("a", "x", greedy()), Turn("b", "x", greedy(logit_bias={3: -100.0}))
    assert e.dist_greedy([plain, plain]) is True
    assert e.dist_greedy([plain, banned]) is False


# ---- a stub model with exact-arithmetic logits: the chunked decode -------------------------------

LEVELS = [5.0 - 0.75 * i for i in range(8)]         # distinct modulo 2: frequency_penalty 2 never ties them
HOT = [11, 23, 5, 40, 17, 30, 2, 9]


def stub_logits(engine):
    """Every forward returns the same row: HOT[i] at LEVELS[i], the rest at -8."""
    row = torch.full((engine.cfg.vocab,), -8.0)
    row[HOT] = torch.tensor(LEVELS)
    real = engine.model.forward

    def forward(*a, **k):
        out = real(*a, **k)
        return row.to(out.dtype).expand(out.shape[0], -1).clone()
    engine.model.forward = forward


def expected_with_frequency_penalty(n, fp):
    count, ids = {}, []
    for _ in range(n):
        score = {t: v - fp * count.get(t, 0) for t, v in zip(HOT, LEVELS)}
        best = max(score, key=score.get)
        assert sorted(score.values())[-1] > sorted(score.values())[-2]
        ids.append(best)
        count[best] = count.get(best, 0) + 1
    return ids


def test_stub_run_turns_counts_the_reply():
    e = cpu_engine()
    stub_logits(e)
    want = expected_with_frequency_penalty(14, 2.0)
    assert want[:4] == [11, 23, 5, 11] and len(set(want)) < len(want)
    assert e.run_turns([Turn("K", PROMPT, greedy(14, frequency_penalty=2.0))])[0].ids == want
    assert e.run_turns([Turn("K0", PROMPT, greedy(14))])[0].ids == [11] * 14


def test_chunked_decode_carries_the_reply_across_chunks():
    """start_turns + continue_decode in chunks of 4 (what serve's scheduler does): tokens generated
    in chunk 1 are counted in chunk 2 and later."""
    e = cpu_engine()
    stub_logits(e)
    want = expected_with_frequency_penalty(13, 2.0)
    turn = Turn("S", PROMPT, greedy(13, frequency_penalty=2.0))
    (sq, first, _), = e.start_turns([turn])
    assert sq.reply_start == sq.length
    gen = [first]
    while len(gen) < 13:
        gen += e.continue_decode([sq], [turn], [gen[-1]], 4)[0]
    assert gen == want
    # the prompt's tokens are not counted: only the reply is
    assert sq.reply_start == len(e.encode_prompt(PROMPT))


def test_serve_chunked_decode_through_http():
    srv = build_server("tiny-llama", weights="random:1", device="cpu", port=0, max_batch=4, max_tokens=16,
                       num_blocks=256).start()
    try:
        srv.sched.chunk = 4
        stub_logits(srv.engine)
        out, _ = srv.generate("Onderwerp:", {"max_tokens": 13, "temperature": 0, "frequency_penalty": 2.0,
                                             "ignore_eos": True}, None)
        assert out.ids == expected_with_frequency_penalty(13, 2.0)
    finally:
        srv.close()


# ---- serve ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def server():
    srv = build_server("tiny-llama", weights="random:1", device="cpu", port=0, max_batch=4, max_tokens=8,
                       num_blocks=256).start()
    yield srv
    srv.close()


def _stream_text(url, body, path="/v1/completions"):
    req = urllib.request.Request(url + path, data=json.dumps(dict(body, stream=True)).encode(), method="POST",
                                 headers={"Content-Type": "application/json"})
    text = ""
    with urllib.request.urlopen(req, timeout=120) as r:
        assert r.status == 200
        for raw in r:
            line = raw.decode().strip()
            if line.startswith("data: ") and line != "data: [DONE]":
                text += json.loads(line[6:])["choices"][0]["text"]
    return text


def test_openai_logit_bias_bans_streamed_and_not(server):
    body = {"prompt": "Onderwerp: caching.", "max_tokens": 8, "temperature": 0, "ignore_eos": True}
    base, _ = server.generate(body["prompt"], body, None)
    assert len(base.ids) == 8
    banned_body = dict(body, logit_bias={str(a): -100 for a in set(base.ids)})       # OpenAI: string keys
    banned, r = server.generate(body["prompt"], banned_body, None)
    assert r.params.logit_bias == {a: -100.0 for a in set(base.ids)}
    assert len(banned.ids) == 8 and not set(banned.ids) & set(base.ids)
    code, reply = _post(server.url + "/v1/completions", banned_body)
    assert code == 200 and json.loads(reply)["choices"][0]["text"] == banned.text != base.text
    assert _stream_text(server.url, banned_body) == banned.text
    # the chat route takes the same fields
    chat = {"messages": [{"role": "user", "content": "Hallo"}], "max_tokens": 4, "temperature": 0,
            "presence_penalty": 0.5, "frequency_penalty": 0.5, "repetition_penalty": 1.2, "repeat_last_n": 32}
    assert _post(server.url + "/v1/chat/completions", chat)[0] == 200
    p = server.sampling(chat)
    assert (p.presence_penalty, p.frequency_penalty, p.repetition_penalty, p.repeat_last_n) == (0.5, 0.5, 1.2, 32)


def test_ollama_options_mapping(server, monkeypatch):
    seen = []
    real = server.sampling
    monkeypatch.setattr(server, "sampling", lambda body: seen.append(real(body)) or seen[-1])
    msgs = [{"role": "user", "content": "q"}]
    code, _ = _post(server.url + "/api/chat", {"messages": msgs, "stream": False, "options": {
        "num_predict": 3, "temperature": 0, "repeat_penalty": 1.3, "repeat_last_n": -1, "presence_penalty": 0.25,
        "frequency_penalty": -0.5}})
    assert code == 200
    p = seen[-1]
    assert (p.repetition_penalty, p.repeat_last_n, p.presence_penalty, p.frequency_penalty) == (1.3, -1, 0.25, -0.5)
    assert p.has_processors()
    # a request that sends none of them is neutral: Ollama's own 1.1 default is not adopted
    _post(server.url + "/api/chat", {"messages": msgs, "stream": False, "options": {"num_predict": 3}})
    assert not seen[-1].has_processors() and seen[-1].repetition_penalty == 1.0


BAD = [
    ("presence above 2", {"presence_penalty": 2.5}),
    ("presence below -2", {"presence_penalty": -2.01}),
    ("frequency above 2", {"frequency_penalty": 3}),
    ("frequency below -2", {"frequency_penalty": -3}),
    ("repetition zero", {"repetition_penalty": 0}),
    ("repetition negative", {"repetition_penalty": -1.5}),
    ("301 biases", {"logit_bias": {str(i): 1 for i in range(301)}}),
    ("bias above 100", {"logit_bias": {"5": 100.5}}),
    ("bias below -100", {"logit_bias": {"5": -101}}),
    ("token id past the vocabulary", {"logit_bias": {"99999999": 1}}),
    ("negative token id", {"logit_bias": {"-1": 1}}),
    ("token id not a number", {"logit_bias": {"abc": 1}}),
    ("bias list", {"logit_bias": [1, 2]}),
]


@pytest.mark.parametrize("name,extra", BAD, ids=[b[0] for b in BAD])
def test_invalid_values_get_400(server, name, extra):
    for path, body in (("/v1/completions", {"prompt": "x", "max_tokens": 2}),
                       ("/v1/chat/completions", {"messages": [{"role": "user", "content": "x"}], "max_tokens": 2,
                                                 "stream": True})):
        with pytest.raises(urllib.error.HTTPError) as ei:
            _post(server.url + path, dict(body, **extra))
        assert ei.value.code == 400
        err = json.loads(ei.value.read().decode())["error"]
        assert err["type"] == "invalid_request_error" and err["message"]


def test_invalid_ollama_options_get_400(server):
    for opts in ({"repeat_penalty": 0}, {"presence_penalty": 9}, {"frequency_penalty": -9}):
        with pytest.raises(urllib.error.HTTPError) as ei:
            _post(server.url + "/api/chat", {"messages": [{"role": "user", "content": "q"}], "stream": False,
                                             "options": opts})
        assert ei.value.code == 400


def test_limits_are_accepted(server):
    vocab = int(server.engine.cfg.vocab)
    body = {"prompt": "x", "max_tokens": 2, "presence_penalty": 2, "frequency_penalty": -2,
            "repetition_penalty": 0.01, "logit_bias": {str(i): (100 if i % 2 else -100) for i in range(299)}}
    body["logit_bias"][str(vocab - 1)] = 0
    assert len(body["logit_bias"]) == 300
    assert _post(server.url + "/v1/completions", body)[0] == 200


# ---- knights' config --------------------------------------------------------------------------------

def test_config_schema_takes_the_same_keys():
    assert not SamplingParams(**processor_settings(ENGINE_DEFAULTS)).has_processors()
    got = processor_settings({"repetition_penalty": 1.15, "repeat_last_n": 256, "frequency_penalty": 0.3,
                              "presence_penalty": 0.2, "logit_bias": {"13": -100, "198": 2.5}})
    assert got["logit_bias"] == {13: -100.0, 198: 2.5} and got["repeat_last_n"] == 256
    for bad in ({"presence_penalty": 3}, {"repetition_penalty": 0}, {"logit_bias": {"1": 101}},
                {"logit_bias": {"x": 1}}, {"logit_bias": [1]}):
        with pytest.raises(ConfigError):
            processor_settings(bad)


def test_example_config_builds_a_penalised_knight():
    from theroundtaible_amd.config import engine_settings, validate_config
    from theroundtaible_amd.types import RoundtableConfig
    raw = json.load(open(os.path.join(ROOT, "examples", "config.penalties.json")))
    validate_config(raw)
    cfg = RoundtableConfig.from_dict(raw)
    claude = SamplingParams(**processor_settings(engine_settings(cfg, "claude-cli")))
    assert claude.has_processors() and claude.logit_bias == {13: -100.0, 198: 2.5}
    assert (claude.repetition_penalty, claude.repeat_last_n) == (1.15, 256)
    assert not SamplingParams(**processor_settings(engine_settings(cfg, "openai-cli"))).has_processors()


# ---- tensor parallel --------------------------------------------------------------------------------

def test_serve_tp2_matches_tp1_under_bans():
    """``serve --tp 2`` over gloo: every rank applies the same processors to its gathered logits, so
    greedy completions with bans equal the tp 1 server's (MirroredEngine mirrors the fields)."""
    prompts = ["De ronde tafel opent de zitting.", "Een korte vraag."]
    ref = build_server("tiny-llama", weights="random-full:1", device="cpu", port=0, max_batch=4, max_tokens=8,
                       num_blocks=256).start()
    try:
        bodies, want, plain = [], [], []
        for p in prompts:
            body = {"prompt": p, "max_tokens": 8, "temperature": 0, "ignore_eos": True}
            base, _ = ref.generate(p, body, None)
            bodies.append(dict(body, logit_bias={str(a): -100 for a in set(base.ids)}, frequency_penalty=1.0))
            out, _ = ref.generate(p, bodies[-1], None)
            assert not set(out.ids) & set(base.ids)
            want.append(out.text)
            plain.append(base.text)
    finally:
        ref.close()
    port = free_port()
    env = dict(os.environ, OMP_NUM_THREADS="1", PYTHONPATH=ROOT)
    p = subprocess.Popen([sys.executable, "-m", "theroundtaible_amd", "serve", "--model", "tiny-llama",
                          "--weights", "random-full:1", "--device", "cpu", "--tp", "2", "--port", str(port),
                          "--max-batch", "4", "--max-tokens", "8", "--num-blocks", "256"],
                         cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         start_new_session=True)
    url = f"http://127.0.0.1:{port}"
    try:
        deadline = time.time() + 180
        while True:
            try:
                with urllib.request.urlopen(url + "/health", timeout=5) as r:
                    if r.status == 200:
                        break
            except OSError:
                pass
            assert p.poll() is None, p.stdout.read()[-3000:]
            assert time.time() < deadline, "tp2 server did not come up"
            time.sleep(0.5)
        got = [json.loads(_post(url + "/v1/completions", b)[1])["choices"][0]["text"] for b in bodies]
        assert got == want and got != plain
        unbanned = json.loads(_post(url + "/v1/completions", {"prompt": prompts[0], "max_tokens": 8, "temperature": 0,
                                                              "ignore_eos": True})[1])["choices"][0]["text"]
        assert unbanned == plain[0]
    finally:
        from test_serve_tp import _stop
        _stop(p)
