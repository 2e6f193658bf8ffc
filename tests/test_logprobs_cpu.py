"""Logprobs on the CPU: the fp32 reference (ops/reference.py) against the fp64 oracle on every kernel
case, the engine's records (run_turns, forced tails, start_turns + chunked continue_decode), the serve
front end over HTTP (both response shapes, the 400s, streaming) and a tp 2 server against tp 1."""
import json
import math
import os
import subprocess
import sys
import time
import urllib.error
import urllib.request

import pytest
import torch

from test_distributed_cpu import ROOT, free_port
from theroundtaible_amd import ops
from theroundtaible_amd.engine import Engine, EngineConfig, SamplingParams, Turn
from theroundtaible_amd.ops import oracle64 as o64
from theroundtaible_amd.serve import build_server

PROMPT = "Hallo tafel, wat is het plan voor vandaag?"
TOL = 1e-4        # engine-level sanity on sums of probabilities, not a kernel tolerance


def greedy(n=10, **kw):
    return SamplingParams(temperature=0.0, max_new_tokens=n, ignore_eos=True, stop_on_consensus=False, **kw)


def _post(url, body):
    req = urllib.request.Request(url, data=json.dumps(body).encode(), method="POST",
                                 headers={"Content-Type": "application/json"})
    with urllib.request.urlopen(req, timeout=120) as r:
        return r.status, r.read().decode()


# ---- reference against oracle -----------------------------------------------------------------------

def _reference_ratio(V, dtype, kind, B=3, ld=None):
    logits, n_top, toks = o64.logprob_case(V, dtype, kind, B=B, ld=ld)
    before = logits.clone()
    lp = ops.LogProbs(B, "cpu", 1)
    lp.n_top.copy_(n_top)
    ops.token_logprobs(logits, lp, ids=toks)
    assert torch.equal(logits.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       before.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    oracle = o64.token_logprobs(logits, n_top, toks)
    return o64.assert_logprobs(lp.tok_lp[0], lp.top_id[0], lp.top_lp[0], oracle, n_top, f"V={V} {dtype} {kind}")


def test_reference_vs_oracle(capsys):
    """Every kernel case of tests/test_logprobs_gpu.py: ids exactly, values within logprob_tol. The
    worst ratio, rescaled, is the measurement LOGPROB_SLACK was derived from (4x, next power of two)."""
    worst = 0.0
    for dtype in (torch.bfloat16, torch.float32):
        for V in o64.LOGPROB_V:
            for kind in o64.LOGPROB_KINDS:
                if kind == "big80" and dtype != torch.float32:
                    continue
                worst = max(worst, _reference_ratio(V, dtype, kind, ld=1008 if V == 1003 else None))
        worst = max(worst, _reference_ratio(o64.LOGPROB_V_BIG, dtype, "random"))
        for kind in ("random", "levels8"):
            worst = max(worst, _reference_ratio(4097, dtype, kind, B=32))
    with capsys.disabled():
        print(f"\nRATIO logprobs reference worst {worst:.3f} = {worst * o64.LOGPROB_SLACK:.3e} * (1 + |l| + |lse|)")
    assert worst * o64.LOGPROB_SLACK <= o64.LOGPROB_REF_WORST * 1.0001, "LOGPROB_REF_WORST is not the measured worst"
    assert o64.LOGPROB_SLACK == 2.0 ** math.ceil(math.log2(4 * o64.LOGPROB_REF_WORST))


def test_tie_rule_and_tail():
    lp = ops.LogProbs(2, "cpu", 1)
    lp.n_top.copy_(torch.tensor([20, 3], dtype=torch.int32))
    logits = torch.tensor([[1.0, 2.0, 2.0, -0.0, 0.0], [0.5, float("-inf"), 0.5, 0.5, float("-inf")]])
    ops.token_logprobs(logits, lp, ids=torch.tensor([1, 7]))
    assert lp.top_id[0, 0].tolist() == [1, 2, 0, 3, 4] + [-1] * 15       # value descending, then id ascending
    assert bool((lp.top_lp[0, 0, 5:] == -math.inf).all())
    assert lp.top_id[0, 1, :3].tolist() == [0, 2, 3] and math.isnan(float(lp.tok_lp[0, 1]))
    assert abs(float(lp.top_lp[0, 1, 0]) + math.log(3)) < 1e-6
    with pytest.raises(ValueError):
        ops.token_logprobs(logits, lp)
    with pytest.raises(ValueError):
        ops.LogProbs(1, "cpu").fill([SamplingParams(logprobs=21)])


def test_sampling_params():
    assert SamplingParams().logprobs is None and not SamplingParams().wants_logprobs()
    assert SamplingParams(logprobs=0).wants_logprobs()
    SamplingParams(logprobs=20).check_logprobs()
    for bad in (-1, 21, 1.5, True):
        with pytest.raises(ValueError):
            SamplingParams(logprobs=bad).check_logprobs()
    assert ops.MAX_TOP_LOGPROBS == 20


# ---- engine (the examples/config.cpu-gpt2.json shape) ---------------------------------------------

@pytest.fixture(scope="module")
def engine():
    return Engine(EngineConfig(model="gpt2-small", device="cpu", dtype="fp32", num_blocks=128, weights="random:1"))


def test_engine_records(engine):
    base = engine.run_turns([Turn("K1", PROMPT, greedy())])[0]
    assert base.error is None and base.logprobs is None
    out = engine.run_turns([Turn("K2", PROMPT, greedy(logprobs=5))])[0]
    assert out.error is None and out.ids == base.ids, "logprobs changed the sampled ids"
    assert len(out.logprobs) == len(out.ids) == 10
    for tok, (tok_lp, top_ids, top_lps) in zip(out.ids, out.logprobs):
        assert len(top_ids) == len(top_lps) == 5
        assert top_ids[0] == tok and tok_lp == top_lps[0], "a greedy row's token is its most likely one"
        assert top_lps == sorted(top_lps, reverse=True)
        assert sum(math.exp(v) for v in top_lps) <= 1 + TOL
    # logprobs=0: the chosen token's logprob alone
    zero = engine.run_turns([Turn("K3", PROMPT, greedy(logprobs=0))])[0]
    assert [r[0] for r in zero.logprobs] == [r[0] for r in out.logprobs] and all(r[1] == [] for r in zero.logprobs)


def test_engine_mixed_batch_and_sampled_rows(engine):
    sampled = SamplingParams(temperature=0.9, top_p=0.9, seed=3, max_new_tokens=8, ignore_eos=True,
                             stop_on_consensus=False)
    plain = engine.run_turns([Turn("M1", PROMPT, sampled), Turn("M2", PROMPT + " Anders.", greedy(8))])
    for k in ("M1", "M2"):          # the RNG is keyed by (seed, sequence key, position): same keys, fresh sequences
        engine.release(k)
    both = engine.run_turns([Turn("M1", PROMPT, SamplingParams(**{**sampled.__dict__, "logprobs": 20})),
                             Turn("M2", PROMPT + " Anders.", greedy(8))])
    assert [o.ids for o in both] == [o.ids for o in plain]
    assert both[1].logprobs is None and len(both[0].logprobs) == 8
    for tok, (tok_lp, top_ids, top_lps) in zip(both[0].ids, both[0].logprobs):
        assert tok_lp <= top_lps[0] <= 0.0
        if tok in top_ids:
            assert top_lps[top_ids.index(tok)] == tok_lp


def test_engine_forced_tail_gives_none_entries(engine):
    out = engine.run_turns([Turn("F", PROMPT, greedy(4, logprobs=2, forced_tail=" ok dan"))])[0]
    n_tail = int(out.metrics["forced_tokens"])
    assert n_tail > 0 and len(out.logprobs) == len(out.ids) == 4 + n_tail
    assert all(r is not None for r in out.logprobs[:4]) and out.logprobs[4:] == [None] * n_tail


def test_chunked_decode_yields_the_same_records(engine):
    whole = engine.run_turns([Turn("W", PROMPT, greedy(10, logprobs=5))])[0]
    turn = Turn("S", PROMPT, greedy(10, logprobs=5))
    (sq, first, _), = engine.start_turns([turn])
    assert len(sq.reply_logprobs) == 1
    gen = [first]
    while len(gen) < 10:
        gen += engine.continue_decode([sq], [turn], [gen[-1]], 3)[0]
        assert len(sq.reply_logprobs) == len(gen)
    assert gen[:10] == whole.ids
    assert sq.reply_logprobs[:10] == whole.logprobs
    (sq2, _, _), = engine.start_turns([Turn("S2", PROMPT, greedy(10))])
    assert sq2.reply_logprobs is None


def test_dist_greedy_is_off_for_a_batch_with_logprobs():
    from theroundtaible_amd.parallel.tp import TPInfo
    e = object.__new__(Engine)
    e.tp = TPInfo(size=2, rank=0)
    e.on_gpu = False
    e.ecfg = EngineConfig(device="cpu")
    plain, asking = Turn("a", "x", greedy()), Turn("b", "x", greedy(logprobs=0))
    assert e.dist_greedy([plain, plain]) is True
    assert e.dist_greedy([plain, asking]) is False


# ---- serve -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def server():
    srv = build_server("tiny-llama", weights="random:1", device="cpu", port=0, max_batch=4, max_tokens=8,
                       num_blocks=256).start()
    srv.sched.chunk = 3         # several decode chunks per reply: streamed pieces
    yield srv
    srv.close()


CHAT = {"messages": [{"role": "user", "content": "Hallo"}], "max_tokens": 7, "temperature": 0, "ignore_eos": True}
COMP = {"prompt": "Onderwerp: caching.", "max_tokens": 7, "temperature": 0, "ignore_eos": True}


def test_chat_completions_shape(server):
    code, reply = _post(server.url + "/v1/chat/completions", dict(CHAT, logprobs=True, top_logprobs=5))
    assert code == 200
    d = json.loads(reply)
    content = d["choices"][0]["logprobs"]["content"]
    assert len(content) == d["usage"]["completion_tokens"] == 7
    assert "".join(e["token"] for e in content) == d["choices"][0]["message"]["content"]
    for e in content:
        assert set(e) == {"token", "logprob", "bytes", "top_logprobs"} and e["bytes"] == list(e["token"].encode())
        assert len(e["top_logprobs"]) == 5 and all(set(t) == {"token", "logprob", "bytes"} for t in e["top_logprobs"])
        assert e["top_logprobs"][0]["token"] == e["token"] and e["top_logprobs"][0]["logprob"] == e["logprob"]
        assert e["logprob"] <= 0 and sum(math.exp(t["logprob"]) for t in e["top_logprobs"]) <= 1 + TOL
    # logprobs: true alone: no alternatives
    d0 = json.loads(_post(server.url + "/v1/chat/completions", dict(CHAT, logprobs=True))[1])
    assert [e["logprob"] for e in d0["choices"][0]["logprobs"]["content"]] == [e["logprob"] for e in content]
    assert all(e["top_logprobs"] == [] for e in d0["choices"][0]["logprobs"]["content"])


def test_completions_legacy_shape(server):
    d = json.loads(_post(server.url + "/v1/completions", dict(COMP, logprobs=3))[1])
    lp = d["choices"][0]["logprobs"]
    assert set(lp) == {"tokens", "token_logprobs", "top_logprobs", "text_offset"}
    assert len(lp["tokens"]) == len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == len(lp["text_offset"]) == 7
    assert "".join(lp["tokens"]) == d["choices"][0]["text"]
    assert lp["text_offset"] == [sum(len(t) for t in lp["tokens"][:i]) for i in range(7)]
    for tok, v, top in zip(lp["tokens"], lp["token_logprobs"], lp["top_logprobs"]):
        assert isinstance(top, dict) and 1 <= len(top) <= 3 and top[tok] == v == max(top.values())


def test_no_logprobs_key_unless_asked(server):
    d = json.loads(_post(server.url + "/v1/completions", COMP)[1])
    assert list(d["choices"][0]) == ["index", "text", "finish_reason"]
    d = json.loads(_post(server.url + "/v1/chat/completions", CHAT)[1])
    assert list(d["choices"][0]) == ["index", "message", "finish_reason"]
    d = json.loads(_post(server.url + "/v1/chat/completions", dict(CHAT, logprobs=False))[1])
    assert "logprobs" not in d["choices"][0]
    # the same ids with and without
    a, _ = server.generate(COMP["prompt"], COMP, None)
    b, _ = server.generate(COMP["prompt"], dict(COMP, logprobs=4), None)
    assert a.ids == b.ids and a.logprobs is None and len(b.logprobs) == len(b.ids)


BAD = [
    ("chat: top_logprobs without logprobs", "/v1/chat/completions", {"top_logprobs": 3}),
    ("chat: top_logprobs with logprobs false", "/v1/chat/completions", {"logprobs": False, "top_logprobs": 3}),
    ("chat: top_logprobs 21", "/v1/chat/completions", {"logprobs": True, "top_logprobs": 21}),
    ("chat: top_logprobs -1", "/v1/chat/completions", {"logprobs": True, "top_logprobs": -1}),
    ("chat: top_logprobs not an integer", "/v1/chat/completions", {"logprobs": True, "top_logprobs": "3"}),
    ("chat: logprobs an integer", "/v1/chat/completions", {"logprobs": 3}),
    ("completions: logprobs 21", "/v1/completions", {"logprobs": 21}),
    ("completions: logprobs -1", "/v1/completions", {"logprobs": -1}),
    ("completions: logprobs a boolean", "/v1/completions", {"logprobs": True}),
    ("completions: echo with logprobs", "/v1/completions", {"logprobs": 2, "echo": True}),
]


@pytest.mark.parametrize("name,path,extra", BAD, ids=[b[0] for b in BAD])
def test_invalid_requests_get_400(server, name, path, extra):
    body = dict(CHAT if "chat" in path else COMP, **extra)
    for stream in (False, True):
        with pytest.raises(urllib.error.HTTPError) as ei:
            _post(server.url + path, dict(body, stream=stream))
        assert ei.value.code == 400
        err = json.loads(ei.value.read().decode())["error"]
        assert err["type"] == "invalid_request_error" and err["message"]


def _stream(url, path, body):
    req = urllib.request.Request(url + path, data=json.dumps(dict(body, stream=True)).encode(), method="POST",
                                 headers={"Content-Type": "application/json"})
    chunks = []
    with urllib.request.urlopen(req, timeout=120) as r:
        assert r.status == 200
        for raw in r:
            line = raw.decode().strip()
            if line.startswith("data: ") and line != "data: [DONE]":
                chunks.append(json.loads(line[6:])["choices"][0])
    return chunks


def test_streamed_entries_concatenate_to_the_list(server):
    whole = json.loads(_post(server.url + "/v1/chat/completions", dict(CHAT, logprobs=True, top_logprobs=2))[1])
    chunks = _stream(server.url, "/v1/chat/completions", dict(CHAT, logprobs=True, top_logprobs=2))
    with_lp = [c for c in chunks if "logprobs" in c]
    assert len(with_lp) >= 2, "the reply came in one piece: nothing was streamed"
    got = [e for c in with_lp for e in c["logprobs"]["content"]]
    assert got == whole["choices"][0]["logprobs"]["content"]
    assert "".join(c["delta"].get("content", "") for c in chunks) == whole["choices"][0]["message"]["content"]
    # legacy shape: the lists concatenate, the offsets run on
    whole = json.loads(_post(server.url + "/v1/completions", dict(COMP, logprobs=2))[1])["choices"][0]["logprobs"]
    chunks = [c for c in _stream(server.url, "/v1/completions", dict(COMP, logprobs=2)) if "logprobs" in c]
    assert len(chunks) >= 2
    for key in ("tokens", "token_logprobs", "top_logprobs", "text_offset"):
        assert [x for c in chunks for x in c["logprobs"][key]] == whole[key], key
    # a stream that did not ask carries no logprobs key
    assert all("logprobs" not in c for c in _stream(server.url, "/v1/completions", COMP))


def test_stop_string_list_covers_the_kept_ids(server):
    base, _ = server.generate(COMP["prompt"], dict(COMP, logprobs=1), None)
    stop = server.engine.tokenizer.decode(base.ids[3:4])
    assert stop and stop not in server.engine.tokenizer.decode(base.ids[:3])
    out, r = server.generate(COMP["prompt"], dict(COMP, logprobs=1, stop=[stop]), None)
    assert out.metrics["stop_string"] and len(out.logprobs) == len(out.ids) >= 4
    assert out.logprobs == base.logprobs[:len(out.ids)]


def test_minus_infinity_is_serialised_as_minus_9999(server):
    got = server.logprobs_json([5], [(float("-inf"), [5, 6], [float("-inf"), float("nan")])], chat=True)
    assert got["content"][0]["logprob"] == -9999.0
    assert [t["logprob"] for t in got["content"][0]["top_logprobs"]] == [-9999.0, -9999.0]
    json.loads(json.dumps(got, allow_nan=False))


# ---- tensor parallel -------------------------------------------------------------------------------

def test_serve_tp2_matches_tp1_with_logprobs():
    """``serve --tp 2`` over gloo: a batch that asks for logprobs gathers full logits on every rank, so
    greedy completions with logprobs=3 equal the tp 1 server's: ids equal, values within tolerance."""
    prompts = ["De ronde tafel opent de zitting.", "Een korte vraag."]
    bodies = [{"prompt": p, "max_tokens": 8, "temperature": 0, "ignore_eos": True, "logprobs": 3} for p in prompts]
    ref = build_server("tiny-llama", weights="random-full:1", device="cpu", port=0, max_batch=4, max_tokens=8,
                       num_blocks=256).start()
    try:
        want = [json.loads(_post(ref.url + "/v1/completions", b)[1])["choices"][0] for b in bodies]
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
        got = [json.loads(_post(url + "/v1/completions", b)[1])["choices"][0] for b in bodies]
        for g, w in zip(got, want):
            assert g["text"] == w["text"] and g["logprobs"]["tokens"] == w["logprobs"]["tokens"]
            assert len(g["logprobs"]["token_logprobs"]) == 8
            # tp 2 sums each row-parallel GEMM in two halves: fp32 logits differ in the last bits
            for a, b in zip(g["logprobs"]["token_logprobs"], w["logprobs"]["token_logprobs"]):
                assert abs(a - b) <= 1e-3 * (1 + abs(b))
            for a, b in zip(g["logprobs"]["top_logprobs"], w["logprobs"]["top_logprobs"]):
                assert list(a) == list(b)
                assert all(abs(a[k] - b[k]) <= 1e-3 * (1 + abs(b[k])) for k in a)
    finally:
        from test_serve_tp import _stop
        _stop(p)


# ---- the launcher's plan (csrc/logprobs_plan.h), on the host ---------------------------------------

def test_launch_plan_rules_on_the_host(tmp_path):
    """Chunk counts, workspace size and every refusal of the launcher, compiled as a host program
    with the undefined-behaviour and address sanitizers (the header holds no device code)."""
    import shutil
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "logprobs_plan_check")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "csrc", "tests", "logprobs_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "0 failure(s)" in r.stdout, r.stdout + r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
