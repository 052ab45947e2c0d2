"""Sampler controls on the CPU path (docs/sampling.md): the fp32 reference chain on
hand-computed rows (logit_bias -> repeat / presence / frequency penalty -> top-k -> softmax ->
top-p -> min-p), the Sampler's routing, the engine predicates, the split-server wire and the
ranges each HTTP route enforces."""
import math

import msgpack
import numpy as np
import pytest
import torch
from fastapi.testclient import TestClient

from llm_kubernetes_minikube_sharp4dev_amd import ops
from llm_kubernetes_minikube_sharp4dev_amd.config import Config
from llm_kubernetes_minikube_sharp4dev_amd.engine.llm_engine import LLMEngine, _jump_ok, _plain_greedy
from llm_kubernetes_minikube_sharp4dev_amd.engine.sampling import Sampler, SamplingParams
from llm_kubernetes_minikube_sharp4dev_amd.models import build_decoder
from llm_kubernetes_minikube_sharp4dev_amd.ops import reference as ref
from llm_kubernetes_minikube_sharp4dev_amd.serving.engine_core import SP_FIELDS, sp_to_wire
from llm_kubernetes_minikube_sharp4dev_amd.serving.model_manager import ModelManager
from llm_kubernetes_minikube_sharp4dev_amd.serving.ollama_server import create_app

ALIASES = {"llama3.1:8b": "llama-tiny", "nomic-embed-text": "bert-tiny"}
MODEL = "llama3.1:8b"
INF = float("inf")


def _prm(B, temp=0.0, top_k=0, top_p=1.0, pen=1.0, last_n=64, reset=0, min_p=0.0, presence=0.0, frequency=0.0,
         width=12, seeds=None):
    prm = np.zeros((B, width), dtype=np.int32)
    f = prm.view(np.float32)
    f[:, 0], f[:, 1], f[:, 2] = temp, top_p, pen
    prm[:, 3], prm[:, 4] = top_k, last_n
    prm[:, 5] = np.arange(B)
    prm[:, 6] = reset
    prm[:, 7] = np.arange(B) if seeds is None else seeds
    if width == 12:
        f[:, 8], f[:, 9], f[:, 10] = min_p, presence, frequency
    return torch.from_numpy(prm)


def _csr(rows: list) -> torch.Tensor:
    """[B+1 offsets | n ids | n f32 bits] of one {id: value} dict (or None) per row."""
    offs, ids, vals = [0], [], []
    for d in rows:
        for t, v in (d or {}).items():
            ids.append(t)
            vals.append(v)
        offs.append(len(ids))
    return torch.from_numpy(np.concatenate([np.asarray(offs, np.int32), np.asarray(ids, np.int32),
                                            np.asarray(vals, np.float32).view(np.int32)]))


# --------------------------------------------------------------------------- reference chain
# V = 33; a ring of W = 8 that has seen 11 tokens (so it wrapped): token 7 three times within the
# last 5 entries and once more outside them, 6 and 9 once within them, 4 and 5 only outside
V, W = 33, 8
SEQ = [1, 2, 3, 7, 4, 5, 7, 6, 7, 9, 7]


def _ring():
    hist = torch.zeros(1, W, dtype=torch.int32)
    for i, t in enumerate(SEQ):
        hist[0, i % W] = t
    return hist, torch.tensor([len(SEQ)], dtype=torch.int32)


def _base():
    return (torch.arange(V, dtype=torch.float32) * 0.5 - 3.0)[None].clone()  # l[6] = 0, l[7] = .5, l[9] = 1.5


def _edited(bias=None, **kw):
    """The row's logits after the reference's bias and penalties (a greedy row), and its token."""
    hist, hl = _ring()
    lg = _base()
    tok = ref.sample(lg, _prm(1, **kw), hist, hl, 0, bias)
    assert int(hl[0]) == (1 if kw.get("reset") else len(SEQ) + 1)
    return lg[0], int(tok[0])


def _expect(changes: dict):
    want = _base()[0]
    for t, v in changes.items():
        want[t] = v
    return want


def test_reference_frequency_only():
    got, _ = _edited(frequency=0.25, last_n=5)
    assert torch.equal(got, _expect({7: 0.5 - 3 * 0.25, 6: 0.0 - 0.25, 9: 1.5 - 0.25}))
    # the whole ring (-1): the fourth 7 and the two tokens outside the last five count too
    got, _ = _edited(frequency=0.25, last_n=-1)
    assert torch.equal(got, _expect({7: 0.5 - 4 * 0.25, 6: -0.25, 9: 1.25, 4: -1.0 - 0.25, 5: -0.5 - 0.25}))


def test_reference_presence_only_applies_with_repeat_penalty_one():
    got, _ = _edited(pen=1.0, presence=0.5, last_n=5)
    assert torch.equal(got, _expect({7: 0.0, 6: -0.5, 9: 1.0}))


def test_reference_all_three_penalties():
    got, tok = _edited(pen=2.0, presence=0.5, frequency=0.25, last_n=5)
    # rp: 0.5 / 2, 0 * 2, 1.5 / 2; then - (c * 0.25 + 0.5)
    assert torch.equal(got, _expect({7: 0.25 - 1.25, 6: 0.0 - 0.75, 9: 0.75 - 0.75}))
    assert tok == V - 1
    # a negative logit is multiplied: the window reaches tokens 4 and 5 (both < 0) with last_n = 8
    got, _ = _edited(pen=2.0, presence=0.5, frequency=0.25, last_n=8)
    assert got[4].item() == -2.0 - 0.75 and got[5].item() == -1.0 - 0.75 and got[7].item() == 0.25 - 1.5


def test_reference_window_off_and_reset_apply_nothing():
    for kw in ({"last_n": 0}, {"reset": 1, "last_n": 5}):
        got, tok = _edited(pen=2.0, presence=0.5, frequency=0.25, **kw)
        assert torch.equal(got, _base()[0]) and tok == V - 1


def test_reference_bias():
    hist, hl = _ring()
    lg = _base()
    lg[0, 3] = -INF
    # ids 33, -1 and 1000 are outside the row: ignored; the masked entry stays masked
    bias = _csr([{3: 100.0, 10: 7.5, V: 50.0, -1: 50.0, 1000: 50.0, 12: -2.0}])
    tok = ref.sample(lg, _prm(1, last_n=0, width=8), hist, hl, 0, bias)
    want = _base()[0]
    want[3], want[10], want[12] = -INF, 2.0 + 7.5, 3.0 - 2.0
    assert torch.equal(lg[0], want) and int(tok[0]) == V - 1
    # the bias lands before the penalties: rp sees the biased logit
    got, _ = _edited(bias=_csr([{7: 3.5}]), pen=2.0, presence=0.5, frequency=0.25, last_n=5)
    assert got[7].item() == (0.5 + 3.5) / 2 - 1.25
    # a row without entries next to one with: only the second row changes
    lg2 = _base().repeat(2, 1)
    h2, l2 = torch.zeros(2, W, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    out = ref.sample(lg2, _prm(2, last_n=0), h2, l2, 0, _csr([None, {5: 100.0}]))
    assert out.tolist() == [V - 1, 5] and torch.equal(lg2[0], _base()[0]) and lg2[1, 5].item() == 99.5


def test_reference_rejects_other_widths():
    hist, hl = _ring()
    with pytest.raises(ValueError):
        ref.sample(_base(), torch.zeros(1, 10, dtype=torch.int32), hist, hl)
    with pytest.raises(ValueError):
        ref.sample(_base(), _prm(1), hist, hl, 0, torch.zeros(3, dtype=torch.int32))


@pytest.mark.parametrize("min_p,top_p,support", [(0.2, 1.0, 3), (0.2, 0.6, 2), (1.0, 1.0, 1), (0.0, 1.0, 16)])
def test_reference_min_p_support(min_p, top_p, support):
    """p = 0.5, 0.25, 0.125, ...: min_p 0.2 keeps 1, .5, .25 (relative to the top), top_p 0.6 cuts
    the third (0.75 of the mass lies before it), min_p 1 keeps the top only."""
    Vn, B = 16, 600
    lg = (-math.log(2.0) * torch.arange(Vn, dtype=torch.float32))[None].repeat(B, 1)
    hist, hl = torch.zeros(B, 4, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    out = ref.sample(lg, _prm(B, temp=1.0, top_k=0, top_p=top_p, min_p=min_p, reset=1), hist, hl, seed=3)
    seen = set(out.tolist())
    if support < 16:
        assert seen == set(range(support))
    else:
        assert seen >= set(range(5)) and max(seen) > 4  # min_p = 0: the tail is still drawn
    # a greedy row ignores min_p
    g = ref.sample(lg[:1], _prm(1, temp=0.0, min_p=0.9, reset=1), hist, hl)
    assert g.tolist() == [0]


# --------------------------------------------------------------------------- params, wire, predicates
def test_from_ollama_maps_the_options():
    sp = SamplingParams.from_ollama({"min_p": 0.05, "presence_penalty": 1.5, "frequency_penalty": -0.5})
    assert (sp.min_p, sp.presence_penalty, sp.frequency_penalty) == (0.05, 1.5, -0.5)
    d = SamplingParams.from_ollama(None)
    assert (d.min_p, d.presence_penalty, d.frequency_penalty, d.logit_bias) == (0.0, 0.0, 0.0, None)


def test_wire_unchanged_by_default_and_round_trips():
    sp = SamplingParams()
    assert sp_to_wire(sp) == {k: getattr(sp, k) for k in SP_FIELDS}
    assert set(sp_to_wire(sp)) == {"temperature", "top_k", "top_p", "repeat_penalty", "repeat_last_n", "seed",
                                   "max_tokens", "min_tokens", "stop", "ignore_eos"}
    sp = SamplingParams(temperature=0.0, min_p=0.1, presence_penalty=0.5, frequency_penalty=1.25,
                        logit_bias={7: -100.0, 300: 2.5}, max_tokens=9)
    back = SamplingParams(**msgpack.unpackb(msgpack.packb(sp_to_wire(sp), use_bin_type=True), raw=False))
    assert back == sp and back.logit_bias == {7: -100.0, 300: 2.5}
    only = sp_to_wire(SamplingParams(frequency_penalty=1.0))
    assert only["frequency_penalty"] == 1.0 and not {"min_p", "presence_penalty", "logit_bias"} & set(only)


def test_plain_greedy_and_jump_predicates():
    g = SamplingParams.greedy
    assert _plain_greedy(g(4))
    assert not _plain_greedy(g(4, presence_penalty=0.5)) and not _plain_greedy(g(4, frequency_penalty=0.5))
    assert not _plain_greedy(g(4, logit_bias={3: 1.0}))
    assert _plain_greedy(g(4, frequency_penalty=0.5, repeat_last_n=0))  # the window is off: nothing to apply
    assert _plain_greedy(g(4, min_p=0.5))                              # min_p does not apply to greedy rows
    proc = lambda hist: [1, 2]
    assert _jump_ok(g(4, logits_processor=proc)) and _jump_ok(g(4, logits_processor=proc, logit_bias={3: 1.0}))
    assert not _jump_ok(g(4, logits_processor=proc, presence_penalty=0.5))
    assert not _jump_ok(g(4, logits_processor=proc, frequency_penalty=0.5))
    assert _jump_ok(g(4, logits_processor=proc, frequency_penalty=0.5, repeat_last_n=0))


# --------------------------------------------------------------------------- Sampler routing
def test_sampler_routes_and_row_width(monkeypatch):
    calls = []
    real = ops.sample

    def spy(logits, prm, hist, hist_len, seed=0, out=None, bias=None):
        calls.append((tuple(prm.shape), None if bias is None else bias.clone()))
        return real(logits, prm, hist, hist_len, seed, out, bias)

    monkeypatch.setattr(ops, "sample", spy)
    Vs = 64
    lg = torch.arange(Vs, dtype=torch.float32)[None].repeat(2, 1)
    g = SamplingParams.greedy
    smp = Sampler(Vs)
    assert smp(lg.clone(), [g(4), g(4)], [[], []], ["a", "b"]).tolist() == [63, 63] and calls == []
    # Ollama's defaults: the 8-wide rows they always were, no bias operand
    smp(lg.clone(), [SamplingParams(), g(4)], [[], []], ["a", "b"])
    assert calls[-1] == ((2, 8), None)
    # a bias alone routes to the fused sampler, still 8 wide; ids outside the vocabulary are dropped
    ids = smp(lg.clone(), [g(4, logit_bias={5: 100.0, 64: 500.0}), g(4)], [[], []], ["c", "d"])
    assert ids.tolist() == [5, 63] and calls[-1][0] == (2, 8)
    assert calls[-1][1].tolist()[:4] == [0, 1, 1, 5] and calls[-1][1].numel() == 5
    # presence / frequency / min_p: 12-wide rows
    p = g(8, frequency_penalty=1e4, repeat_last_n=-1)
    seen = [int(smp(lg[:1].clone(), [p], [[]], ["e"])[0]) for _ in range(6)]
    assert seen == [63, 62, 61, 60, 59, 58] and calls[-1] == ((1, 12), None)
    smp(lg.clone(), [SamplingParams(temperature=1.0, top_k=0, top_p=1.0, repeat_penalty=1.0, min_p=0.5), g(4)],
        [[], []], ["f", "h"])
    assert calls[-1][0] == (2, 12)
    n = len(calls)
    smp(lg.clone(), [g(4, min_p=0.5), g(4)], [[], []], ["i", "j"])  # greedy: min_p is no filter
    assert len(calls) == n


def test_sampler_logprobs_keep_the_raw_logits_under_a_bias():
    Vs = 64
    lg = torch.arange(Vs, dtype=torch.float32)[None].clone()
    keep = lg.clone()
    smp = Sampler(Vs)
    ids = smp(lg, [SamplingParams.greedy(4, logit_bias={5: 100.0}, logprobs=True, top_logprobs=2)], [[]], ["a"])
    assert ids.tolist() == [5] and torch.equal(lg, keep)
    rows, n, chosen, top_lp, top_id = smp.last_logprobs
    want = torch.log_softmax(keep.double(), dim=-1)
    assert top_id[0].tolist() == [63, 62] and abs(chosen[0].item() - want[0, 5].item()) < 1e-4


def test_grammar_row_with_new_controls_leaves_the_sparse_shortcut():
    Vs = 64
    lg = torch.arange(Vs, dtype=torch.float32)[None].clone()
    allowed = [3, 9, 11]
    smp = Sampler(Vs)
    p = SamplingParams.greedy(4, logits_processor=lambda h: allowed, logit_bias={3: 50.0, 40: 100.0})
    assert smp(lg.clone(), [p], [[]], ["a"]).tolist() == [3]  # 40 is biased up but not allowed


# --------------------------------------------------------------------------- engine (CPU path)
def test_engine_three_requests():
    m = build_decoder("llama-tiny", dtype=torch.float32)
    prompts = [list(range(5, 30)), [7, 8, 9], list(range(100, 140))]

    def run(which):
        eng = LLMEngine(m, None, max_model_len=512, max_num_seqs=8, num_blocks=128, use_graphs=False, eos_ids=set())
        mk = [lambda: SamplingParams.greedy(24, frequency_penalty=1e4, repeat_last_n=-1, ignore_eos=True),
              lambda: SamplingParams.greedy(24, logit_bias={77: 100.0}, ignore_eos=True),
              lambda: SamplingParams.greedy(24, ignore_eos=True)]
        seqs = [eng.add_request(prompts[i], mk[i]()) for i in which]
        while eng.has_work():
            eng.step_pipelined()
        eng.flush()
        return [s.output_ids for s in seqs]

    a, b, c = run([0, 1, 2])
    assert len(a) == 24 and len(set(a)) == 24
    assert b == [77] * 24
    assert c == run([2])[0]


# --------------------------------------------------------------------------- HTTP
@pytest.fixture(scope="module")
def server():
    cfg = Config()
    cfg.engine.max_model_len = 2048
    cfg.engine.default_max_new_tokens = 8
    mgr = ModelManager(cfg, device="cpu", aliases=ALIASES)
    with TestClient(create_app(mgr)) as c:
        yield c, mgr
    mgr.shutdown()


def test_openai_logit_bias_forces_the_token(server):
    c, mgr = server
    h = mgr.generator(MODEL)
    tid = next(t for t in range(60, 400) if t not in h.engine.eos_ids and h.tokenizer.decode([t]).strip())
    r = c.post("/v1/completions", json={"model": MODEL, "prompt": "ciao", "max_tokens": 6, "temperature": 0,
                                        "logit_bias": {str(tid): 100}})
    assert r.status_code == 200, r.text
    assert r.json()["choices"][0]["text"] == h.tokenizer.decode([tid] * 6)
    r = c.post("/v1/chat/completions", json={"model": MODEL, "messages": [{"role": "user", "content": "hi"}],
                                             "max_tokens": 5, "temperature": 0, "logit_bias": {str(tid): 100},
                                             "presence_penalty": 2, "frequency_penalty": -2})
    assert r.status_code == 200, r.text
    assert r.json()["choices"][0]["message"]["content"] == h.tokenizer.decode([tid] * 5)


def test_openai_range_violations(server):
    c, mgr = server
    vocab = int(mgr.generator(MODEL).engine.model.cfg.vocab_size)
    comp = {"model": MODEL, "prompt": "ciao", "max_tokens": 2, "temperature": 0}
    chat = {"model": MODEL, "messages": [{"role": "user", "content": "hi"}], "max_tokens": 2, "temperature": 0}
    bad = [{"presence_penalty": 2.5}, {"presence_penalty": -2.01}, {"frequency_penalty": 3}, {"frequency_penalty": "1"},
           {"frequency_penalty": True}, {"logit_bias": [[1, 2.0]]}, {"logit_bias": {str(i): 1 for i in range(301)}},
           {"logit_bias": {"07": 1}}, {"logit_bias": {"-1": 1}}, {"logit_bias": {"1.0": 1}}, {"logit_bias": {"x": 1}},
           {"logit_bias": {str(vocab): 1}}, {"logit_bias": {"5": 100.5}}, {"logit_bias": {"5": -101}},
           {"logit_bias": {"5": "3"}}, {"logit_bias": {"5": None}}]
    for route, body in (("/v1/completions", comp), ("/v1/chat/completions", chat)):
        for extra in bad:
            r = c.post(route, json={**body, **extra})
            assert r.status_code == 400, (route, extra)
            e = r.json()["error"]
            assert e["type"] == "invalid_request_error" and next(iter(extra)) in e["message"]
        ok = {"presence_penalty": -2, "frequency_penalty": 2, "logit_bias": {str(vocab - 1): -100, "0": 100}}
        assert c.post(route, json={**body, **ok}).status_code == 200
        assert c.post(route, json={**body, "logit_bias": {str(i): 1 for i in range(300)}}).status_code == 200


def test_ollama_range_violations(server):
    c, _ = server
    gen = {"model": MODEL, "prompt": "ciao", "stream": False}
    chat = {"model": MODEL, "messages": [{"role": "user", "content": "hi"}], "stream": False}
    bad = [{"min_p": 1.5}, {"min_p": -0.1}, {"min_p": "0.1"}, {"min_p": None}, {"presence_penalty": "a"},
           {"frequency_penalty": [1]}, {"frequency_penalty": True}]
    for route, body in (("/api/generate", gen), ("/api/chat", chat)):
        for extra in bad:
            r = c.post(route, json={**body, "options": {"num_predict": 2, "temperature": 0, **extra}})
            assert r.status_code == 400 and next(iter(extra)) in r.json()["error"], (route, extra)
        # JSON as Python writes it can carry a non-finite number
        r = c.post(route, content=('{"model": "%s", "prompt": "x", "messages": [{"role": "user", "content": "x"}], "stream": false, '
                                   '"options": {"presence_penalty": Infinity}}' % MODEL).encode())
        assert r.status_code == 400 and "presence_penalty" in r.json()["error"]
        ok = {"min_p": 1, "presence_penalty": -7.5, "frequency_penalty": 30}
        assert c.post(route, json={**body, "options": {"num_predict": 2, "temperature": 0, **ok}}).status_code == 200


def test_ollama_frequency_penalty_reaches_the_sampler(server, monkeypatch):
    c, _ = server
    got = []
    real = Sampler.__call__

    def spy(self, logits, params, histories, keys=None):
        got.extend(params)
        return real(self, logits, params, histories, keys)

    monkeypatch.setattr(Sampler, "__call__", spy)
    body = {"model": MODEL, "prompt": "ciao", "stream": False,
            "options": {"num_predict": 8, "temperature": 0, "repeat_penalty": 1.0, "repeat_last_n": -1}}
    plain = c.post("/api/generate", json=body).json()
    assert got == []  # plain greedy: the sampler is not even called
    body["options"].update(frequency_penalty=1e4, presence_penalty=0.25, min_p=0.05)
    d = c.post("/api/generate", json=body).json()
    assert d["done"] and got and all(p.frequency_penalty == 1e4 and p.presence_penalty == 0.25 and p.min_p == 0.05
                                     for p in got)
    assert d["eval_count"] >= 2 and "response" in plain
