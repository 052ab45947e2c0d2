"""Token log-probabilities on the CPU path: the torch reference against float64, the sampler
(raw distribution, caller's logits untouched, no launch when nobody asks), the engine
(same tokens with and without, step() == step_pipelined()), the split-server wire (a 7th
item element for requesting streams only) and the HTTP shapes of every route."""
import asyncio
import codecs
import json
import os
import tempfile

import pytest
import torch
from fastapi.testclient import TestClient

from llm_kubernetes_minikube_sharp4dev_amd import ops
from llm_kubernetes_minikube_sharp4dev_amd.config import Config
from llm_kubernetes_minikube_sharp4dev_amd.engine.llm_engine import LLMEngine
from llm_kubernetes_minikube_sharp4dev_amd.engine.sampling import Sampler, SamplingParams
from llm_kubernetes_minikube_sharp4dev_amd.models import build_decoder
from llm_kubernetes_minikube_sharp4dev_amd.ops import reference as ref
from llm_kubernetes_minikube_sharp4dev_amd.serving.engine_core import EngineCore, sp_to_wire
from llm_kubernetes_minikube_sharp4dev_amd.serving.fake_core import FakeCore
from llm_kubernetes_minikube_sharp4dev_amd.serving.model_manager import ModelManager
from llm_kubernetes_minikube_sharp4dev_amd.serving.ollama_server import create_app
from llm_kubernetes_minikube_sharp4dev_amd.serving.remote import CoreClient, create_frontend_app

ALIASES = {"llama3.1:8b": "llama-tiny", "nomic-embed-text": "bert-tiny"}
MODEL = "llama3.1:8b"


# --------------------------------------------------------------------------- reference
def _f64(logits, ids, rows, n):
    x = logits.double()[rows]
    lp = torch.log_softmax(x, dim=-1)
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices[:, : min(n, x.shape[1])]
    return lp.gather(1, ids.long()[rows][:, None]).squeeze(1), lp.gather(1, order), order


@pytest.mark.parametrize("V", [12, 1003])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reference_against_float64(V, dtype):
    torch.manual_seed(0)
    x = torch.randn(5, V) * 3
    n = 20
    order = torch.sort(x[1], descending=True, stable=True).indices
    k = min(n, V) - 2
    x[1, order[k - 1: k + 2]] = float(x[1, order[k]])   # a tie across a cut inside the list
    x[2, 3] = x[2, V - 1] = 50.0                         # a tie at the maximum
    x[3, V // 2:] = float("-inf")
    x = x.to(dtype)
    ids = torch.tensor([0, int(order[k]), V - 1, V - 1, 7], dtype=torch.int32)
    rows = [4, 1, 2, 3]
    chosen, top_lp, top_id = ops.token_logprobs(x, ids, torch.tensor(rows, dtype=torch.int32), n)
    want_c, want_lp, want_id = _f64(x, ids, rows, n)
    assert top_id.dtype == torch.int32 and top_lp.shape == (4, min(n, V)) and chosen.shape == (4,)
    assert torch.equal(top_id.long(), want_id)
    assert top_id[2, :2].tolist() == [3, V - 1]
    assert chosen[3].item() == float("-inf")
    fin = torch.isfinite(want_lp)
    assert (top_lp.double()[fin] - want_lp[fin]).abs().max() < 1e-5 and torch.equal(top_lp.double()[~fin], want_lp[~fin])
    assert (chosen.double()[:3] - want_c[:3]).abs().max() < 1e-5
    c0, lp0, id0 = ref.token_logprobs(x, ids, torch.tensor(rows, dtype=torch.int32), 0)
    assert torch.equal(c0, chosen) and lp0.shape == (4, 0) and id0.shape == (4, 0)
    with pytest.raises(ValueError):
        ref.token_logprobs(x, ids, torch.tensor(rows, dtype=torch.int32), 21)


# --------------------------------------------------------------------------- sampler
def test_sampler_reports_the_raw_distribution_and_keeps_the_logits():
    torch.manual_seed(1)
    V = 64
    logits = torch.randn(2, V)
    logits[0, 10], logits[0, 20] = 5.0, 4.9   # row 0: the penalty (1.5) moves the argmax 10 -> 20
    logits[1, 30], logits[1, 31] = 6.0, 5.0   # row 1: the grammar excludes the raw argmax 30
    allowed = [i for i in range(V) if i != 30]
    params = [SamplingParams(temperature=0.0, repeat_penalty=1.5, repeat_last_n=64, logprobs=True, top_logprobs=3),
              SamplingParams.greedy(8, logits_processor=lambda hist: allowed, logprobs=True, top_logprobs=5)]
    smp = Sampler(V)
    keep = logits.clone()
    first = smp(logits, params, [[], []], ["a", "b"])       # the ring of "a" now holds token 10
    assert first.tolist() == [10, 31] and torch.equal(logits, keep)
    ids = smp(logits, params, [[10], [31]], ["a", "b"])
    assert ids.tolist() == [20, 31]
    assert torch.equal(logits, keep)                         # mask and penalty ran on a private copy
    rows, n, chosen, top_lp, top_id = smp.last_logprobs
    assert rows == [0, 1] and n == 5
    want = torch.log_softmax(keep.double(), dim=-1)
    assert abs(chosen[0].item() - want[0, 20].item()) < 1e-5 and abs(chosen[1].item() - want[1, 31].item()) < 1e-5
    assert top_id[0, 0].item() == 10 and top_id[0, 1].item() == 20   # raw order: the penalised token still leads
    assert top_id[1, 0].item() == 30                                  # the masked-out argmax is still listed
    assert abs(top_lp[1, 0].item() - want[1, 30].item()) < 1e-5
    # nobody asks: no result, and the call is the old one
    plain = [SamplingParams.greedy(8), SamplingParams.greedy(8)]
    assert smp(logits.clone(), plain, [[], []], ["c", "d"]).tolist() == [10, 30]
    assert smp.last_logprobs is None


def test_sampler_bf16_logits_are_read_as_stored():
    torch.manual_seed(2)
    logits = (torch.randn(3, 200) * 3).to(torch.bfloat16)
    keep = logits.clone()
    params = [SamplingParams(seed=1), SamplingParams(seed=2, logprobs=True, top_logprobs=4), SamplingParams.greedy(4)]
    smp = Sampler(200)
    ids = smp(logits, params, [[], [], []])
    rows, n, chosen, top_lp, top_id = smp.last_logprobs
    assert rows == [1] and n == 4 and torch.equal(logits.view(torch.int16), keep.view(torch.int16))
    want = torch.log_softmax(keep.double(), dim=-1)
    assert abs(chosen[0].item() - want[1, int(ids[1])].item()) < 1e-5
    assert top_id[0].tolist() == torch.sort(keep[1].float(), descending=True, stable=True).indices[:4].tolist()


# --------------------------------------------------------------------------- engine (CPU path)
@pytest.fixture(scope="module")
def tiny():
    return build_decoder("llama-tiny", dtype=torch.float32)


def _eng(m):
    return LLMEngine(m, None, max_model_len=512, max_num_seqs=8, num_blocks=128, use_graphs=False, eos_ids=set())


PROMPTS = [list(range(5, 30)), [7, 8, 9], list(range(100, 140)), [300, 301]]


def _run(m, mk, pipelined=False):
    eng = _eng(m)
    seqs = [eng.add_request(p, mk(i)) for i, p in enumerate(PROMPTS)]
    while eng.has_work():
        eng.step_pipelined() if pipelined else eng.step()
        assert all(len(s.logprobs) == (len(s.output_ids) if s.params.logprobs else 0) for s in seqs)
    eng.flush()
    return seqs


def test_no_launch_when_nobody_asks(tiny, monkeypatch):
    calls = []
    real = ops.token_logprobs
    monkeypatch.setattr(ops, "token_logprobs", lambda *a, **k: calls.append(1) or real(*a, **k))
    _run(tiny, lambda i: SamplingParams.greedy(6) if i % 2 else SamplingParams(seed=i, max_tokens=6), pipelined=True)
    assert calls == []
    seqs = _run(tiny, lambda i: SamplingParams.greedy(6, logprobs=(i == 2), top_logprobs=2 if i == 2 else 0), pipelined=True)
    assert len(calls) == 6  # one launch per step with a requesting row (the request's six tokens)
    assert [len(s.logprobs) for s in seqs] == [0, 0, 6, 0]


def test_tokens_do_not_depend_on_asking(tiny):
    for base in (lambda **kw: SamplingParams.greedy(8, **kw),
                 lambda **kw: SamplingParams(temperature=0.8, top_k=40, top_p=0.9, repeat_penalty=1.2, seed=11,
                                             max_tokens=8, **kw)):
        off = _run(tiny, lambda i: base())
        on = _run(tiny, lambda i: base(logprobs=True, top_logprobs=4))
        assert [s.output_ids for s in on] == [s.output_ids for s in off]
        assert all(s.logprobs == [] for s in off)
        for s in on:
            for tid, (chosen, top) in zip(s.output_ids, s.logprobs):
                assert chosen <= 0.0 and len(top) == 4 and all(a[1] >= b[1] for a, b in zip(top, top[1:]))
                hit = [lp for i, lp in top if i == tid]
                assert not hit or hit[0] == chosen


def test_step_and_step_pipelined_agree(tiny):
    mk = lambda i: SamplingParams.greedy(8, logprobs=True, top_logprobs=i)
    a, b = _run(tiny, mk), _run(tiny, mk, pipelined=True)
    assert [s.output_ids for s in a] == [s.output_ids for s in b]
    assert [s.logprobs for s in a] == [s.logprobs for s in b]
    assert [len(s.logprobs[0][1]) for s in a] == [0, 1, 2, 3]  # each request's own top_logprobs
    for s in a[1:]:  # greedy, no penalty: the chosen token heads its own list
        assert all(top[0] == (tid, chosen) for tid, (chosen, top) in zip(s.output_ids, s.logprobs))


def test_grammar_request_that_asks_does_not_jump(tiny):
    def proc(hist):
        n = len(hist)
        return [(n * 37 + 11) % 512] if n % 7 in (2, 3, 4) else list(range(1 + (n % 5), 512, 3))

    jumping = _run(tiny, lambda i: SamplingParams.greedy(16, logits_processor=proc), pipelined=True)
    asking = _run(tiny, lambda i: SamplingParams.greedy(16, logits_processor=proc, logprobs=True), pipelined=True)
    assert all(s.jumped > 0 for s in jumping) and all(s.jumped == 0 for s in asking)
    assert [s.output_ids for s in asking] == [s.output_ids for s in jumping]
    assert all(len(s.logprobs) == 16 for s in asking)


# --------------------------------------------------------------------------- split-server wire
def test_wire_params_only_when_asked():
    assert "logprobs" not in sp_to_wire(SamplingParams()) and "top_logprobs" not in sp_to_wire(SamplingParams())
    d = sp_to_wire(SamplingParams(logprobs=True, top_logprobs=3))
    assert d["logprobs"] is True and d["top_logprobs"] == 3
    sp = SamplingParams(**d)
    assert sp.logprobs and sp.top_logprobs == 3


def test_fake_core_seventh_element_only_for_requesting_streams():
    import msgpack

    from llm_kubernetes_minikube_sharp4dev_amd.serving.engine_core import _HDR

    path = os.path.join(tempfile.mkdtemp(), "fake.sock")

    async def go():
        core = FakeCore(path, tokens=5, step_s=0.001)
        await core.start()
        # the raw frames: rid 1 asks, rid 2 does not
        reader, writer = await asyncio.open_unix_connection(path)
        for rid, sp in ((1, SamplingParams(max_tokens=5, logprobs=True, top_logprobs=2)), (2, SamplingParams(max_tokens=5))):
            body = msgpack.packb(["gen", rid, "m", [1, 2, 3], sp_to_wire(sp), None], use_bin_type=True)
            writer.write(_HDR.pack(len(body)) + body)
        items, done = [], 0
        while done < 2:
            n = _HDR.unpack(await reader.readexactly(4))[0]
            msg = msgpack.unpackb(await reader.readexactly(n), raw=False)
            assert msg[0] == "tok"
            items += msg[1]
            done += sum(1 for it in msg[1] if it[2])
        writer.close()
        # the front-end's view of the same two requests
        c = CoreClient(path)
        await c.connect()

        async def one(sp):
            view = None
            async for _, _, v in c.stream("m", [1, 2, 3], sp):
                view = v
            return view

        a, b = await asyncio.gather(one(SamplingParams(max_tokens=5, logprobs=True, top_logprobs=2)),
                                    one(SamplingParams(max_tokens=5)))
        c._task.cancel()
        core._server.close()
        return items, a, b

    items, a, b = asyncio.run(go())
    assert {len(it) for it in items if it[0] == 1} == {7} and {len(it) for it in items if it[0] == 2} == {6}
    assert all(len(it[6]) == len(it[1]) for it in items if it[0] == 1)
    assert len(a.output_ids) == 5 and len(a.logprobs) == 5 and b.logprobs == [] and len(b.output_ids) == 5
    assert all(len(top) == 2 and isinstance(chosen, float) for chosen, top in a.logprobs)


def _cfg():
    cfg = Config()
    cfg.engine.max_model_len = 2048
    cfg.engine.default_max_new_tokens = 8
    return cfg


@pytest.fixture(scope="module")
def servers():
    d = tempfile.mkdtemp()
    core_mgr = ModelManager(_cfg(), device="cpu", aliases=ALIASES)
    core = EngineCore(core_mgr, os.path.join(d, "core.sock"))
    local = ModelManager(_cfg(), device="cpu", aliases=ALIASES)
    fe = create_frontend_app([core.path], _cfg(), ALIASES, preload=[MODEL])
    with TestClient(fe) as c_fe, TestClient(create_app(local)) as c_local:
        yield c_fe, c_local
    core.close()
    core_mgr.shutdown()
    local.shutdown()


def test_split_server_answers_like_the_in_process_server(servers):
    c_fe, c_local = servers
    body = {"model": MODEL, "prompt": "ciao", "stream": False, "logprobs": True, "top_logprobs": 3,
            "options": {"num_predict": 6, "temperature": 0}}
    a, b = c_fe.post("/api/generate", json=body).json(), c_local.post("/api/generate", json=body).json()
    assert a["response"] == b["response"] and len(a["logprobs"]) == len(b["logprobs"]) > 0
    for x, y in zip(a["logprobs"], b["logprobs"]):
        assert x["token"] == y["token"] and x["bytes"] == y["bytes"] and abs(x["logprob"] - y["logprob"]) < 1e-4
        assert [t["token"] for t in x["top_logprobs"]] == [t["token"] for t in y["top_logprobs"]]
    plain = {k: v for k, v in body.items() if k not in ("logprobs", "top_logprobs")}
    assert "logprobs" not in c_fe.post("/api/generate", json=plain).json()


# --------------------------------------------------------------------------- HTTP
def _check_entry(e, n):
    assert set(e) == {"token", "logprob", "bytes", "top_logprobs"}
    assert isinstance(e["token"], str) and isinstance(e["logprob"], float) and e["logprob"] <= 0.0
    assert bytes(e["bytes"]).decode("utf-8", errors="replace") == e["token"]
    assert len(e["top_logprobs"]) == n
    for t in e["top_logprobs"]:
        assert set(t) == {"token", "logprob", "bytes"}
    lps = [t["logprob"] for t in e["top_logprobs"]]
    assert all(a >= b for a, b in zip(lps, lps[1:]))


def test_generate_non_streamed(servers):
    _, c = servers
    body = {"model": MODEL, "prompt": "ciao", "stream": False, "logprobs": True, "top_logprobs": 2,
            "options": {"num_predict": 6, "temperature": 0}}
    d = c.post("/api/generate", json=body).json()
    assert d["done"] and len(d["logprobs"]) == d["eval_count"] - (d["done_reason"] == "stop") and len(d["logprobs"]) >= 5
    for e in d["logprobs"]:
        _check_entry(e, 2)
        assert e["top_logprobs"][0]["logprob"] == e["logprob"]  # greedy: the chosen token leads
    body.pop("top_logprobs")
    d0 = c.post("/api/generate", json=body).json()
    assert [e["token"] for e in d0["logprobs"]] == [e["token"] for e in d["logprobs"]]
    assert all(e["top_logprobs"] == [] for e in d0["logprobs"])


def test_generate_streamed(servers):
    _, c = servers
    body = {"model": MODEL, "prompt": "raccontami una storia", "logprobs": True, "top_logprobs": 1,
            "options": {"num_predict": 24, "temperature": 0.9, "seed": 5}}
    with c.stream("POST", "/api/generate", json=body) as r:
        lines = [json.loads(l) for l in r.iter_lines() if l.strip()]
    assert lines[-1]["done"] and all("logprobs" in l for l in lines)
    entries = [e for l in lines for e in l["logprobs"]]
    fin = lines[-1]
    assert len(entries) == fin["eval_count"] - (fin["done_reason"] == "stop") and len(entries) >= 1
    for e in entries:
        _check_entry(e, 1)
    text = "".join(l["response"] for l in lines)
    joined = b"".join(bytes(e["bytes"]) for e in entries)
    # (the server's incremental decoder holds an incomplete trailing UTF-8 sequence back)
    assert codecs.getincrementaldecoder("utf-8")(errors="replace").decode(joined) == text
    # a chunk's entries are the tokens consumed since the previous chunk
    assert all(len(l["logprobs"]) >= 1 for l in lines[:-1])


def test_chat_and_openai_routes(servers):
    _, c = servers
    msgs = [{"role": "user", "content": "hi"}]
    d = c.post("/api/chat", json={"model": MODEL, "messages": msgs, "stream": False, "logprobs": True, "top_logprobs": 2,
                                  "options": {"num_predict": 4, "temperature": 0}}).json()
    assert d["done"] and len(d["logprobs"]) >= 3
    for e in d["logprobs"]:
        _check_entry(e, 2)
    with c.stream("POST", "/api/chat", json={"model": MODEL, "messages": msgs, "logprobs": True,
                                             "options": {"num_predict": 4, "temperature": 0}}) as r:
        lines = [json.loads(l) for l in r.iter_lines() if l.strip()]
    assert [e["token"] for l in lines for e in l["logprobs"]] == [e["token"] for e in d["logprobs"]]

    r = c.post("/v1/chat/completions", json={"model": MODEL, "messages": msgs, "max_tokens": 4, "temperature": 0,
                                             "logprobs": True, "top_logprobs": 3}).json()
    content = r["choices"][0]["logprobs"]["content"]
    assert len(content) >= 3 and len(content) <= r["usage"]["completion_tokens"]
    for e in content:
        _check_entry(e, 3)

    r = c.post("/v1/completions", json={"model": MODEL, "prompt": "ciao", "max_tokens": 5, "temperature": 0,
                                        "logprobs": 2}).json()
    lp = r["choices"][0]["logprobs"]
    assert set(lp) == {"tokens", "token_logprobs", "top_logprobs", "text_offset"}
    n = len(lp["tokens"])
    assert n >= 4 and len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == len(lp["text_offset"]) == n
    assert all(isinstance(t, dict) and 1 <= len(t) <= 2 for t in lp["top_logprobs"])
    assert all(v <= 0.0 for v in lp["token_logprobs"])
    assert lp["text_offset"][0] == 0 and lp["text_offset"] == sorted(lp["text_offset"])


def test_validation_and_unchanged_responses(servers):
    _, c = servers
    msgs = [{"role": "user", "content": "hi"}]
    gen = {"model": MODEL, "prompt": "ciao", "stream": False, "options": {"num_predict": 3, "temperature": 0}}
    chat = {"model": MODEL, "messages": msgs, "stream": False, "options": {"num_predict": 3, "temperature": 0}}
    oa = {"model": MODEL, "messages": msgs, "max_tokens": 3, "temperature": 0}
    for route, body in (("/api/generate", gen), ("/api/chat", chat), ("/v1/chat/completions", oa)):
        assert c.post(route, json={**body, "logprobs": True, "top_logprobs": 21}).status_code == 400
        assert c.post(route, json={**body, "logprobs": True, "top_logprobs": -1}).status_code == 400
        assert c.post(route, json={**body, "top_logprobs": 2}).status_code == 400
        assert c.post(route, json={**body, "logprobs": True, "top_logprobs": 20}).status_code == 200
    comp = {"model": MODEL, "prompt": "ciao", "max_tokens": 3, "temperature": 0}
    assert c.post("/v1/completions", json={**comp, "logprobs": 21}).status_code == 400
    # without the fields: no logprobs key anywhere
    assert "logprobs" not in c.post("/api/generate", json=gen).json()
    assert "logprobs" not in c.post("/api/chat", json=chat).json()
    assert "logprobs" not in c.post("/v1/chat/completions", json=oa).json()["choices"][0]
    assert "logprobs" not in c.post("/v1/completions", json=comp).json()["choices"][0]
    with c.stream("POST", "/api/generate", json={**gen, "stream": True}) as r:
        assert all("logprobs" not in json.loads(l) for l in r.iter_lines() if l.strip())
