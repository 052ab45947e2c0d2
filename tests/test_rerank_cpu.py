"""Cross-encoder reranking without a GPU: the score head's reference (exact probes), HF parity
of CrossEncoderModel, pair tokenisation, the /v1/rerank routes, the split server's rerank op over
a fake core, and the opt-in /rag/search second stage."""
import asyncio
import os
import tempfile
import threading

import numpy as np
import pytest
import torch
from fastapi.testclient import TestClient

import rerank_probes as P
from llm_kubernetes_minikube_sharp4dev_amd import ops
from llm_kubernetes_minikube_sharp4dev_amd.config import Config
from llm_kubernetes_minikube_sharp4dev_amd.models import CrossEncoderModel, build_reranker
from llm_kubernetes_minikube_sharp4dev_amd.models.configs import ENCODERS, RERANKERS, EncoderConfig
from llm_kubernetes_minikube_sharp4dev_amd.models.tokenizer import builtin_tokenizer
from llm_kubernetes_minikube_sharp4dev_amd.serving.model_manager import ModelManager
from llm_kubernetes_minikube_sharp4dev_amd.serving.ollama_server import create_app

ALIASES = {"rr": "rerank-tiny", "emb": "bert-tiny"}


# ------------------------------------------------------------------ the head's reference
@pytest.mark.parametrize("pattern", ["dense", "onehot"])
@pytest.mark.parametrize("H,B", [(128, 1), (384, 3), (64, 9)])
def test_reference_head_exact_probes(pattern, H, B):
    p = P.exact_probe(H, B, pattern)
    assert 0 in P.probe_lens(B) or B == 1
    for fn in (ops.rerank_head, ops.reference.rerank_head):
        got = fn(*P.probe_args(p), 0)
        assert got.dtype == torch.float32 and got.shape == (B,)
        assert np.array_equal(got.numpy().astype(np.int64), p["expected"]) and np.array_equal(
            got.numpy(), p["expected"].astype(np.float32))


def test_reference_head_any_dtype_and_zero_logit():
    p = P.exact_probe(128, 3, "dense", dtype=torch.float32)
    assert np.array_equal(ops.reference.rerank_head(*P.probe_args(p), 0).numpy(), p["expected"].astype(np.float32))
    z = P.zero_logit_probe(128)
    assert ops.rerank_head(*P.probe_args(z), 0).tolist() == [0.0, 0.0]
    assert ops.rerank_head(*P.probe_args(z), 1).tolist() == [0.5, 0.5]
    # no biases, no sequences
    h, cu, w, _, c, _ = P.probe_args(p)
    assert ops.rerank_head(h, cu, w, None, c, None, 0).shape == (3,)
    assert ops.rerank_head(h, cu[:1], w, None, c, None, 0).shape == (0,)


def test_reference_head_within_fp64_bound():
    r = P.random_head(384, 33)
    s64, bound = P.head_fp64(**r)
    got = ops.reference.rerank_head(*P.probe_args(r), 0).double().numpy()
    assert np.all(np.abs(got - s64) <= bound), (np.abs(got - s64).max(), bound.min())


# ------------------------------------------------------------------ model
def _hf(num_labels=1):
    import transformers

    cfg = transformers.BertConfig(vocab_size=300, hidden_size=64, num_hidden_layers=2, num_attention_heads=2,
                                  intermediate_size=128, num_labels=num_labels)
    torch.manual_seed(5)
    return transformers.BertForSequenceClassification(cfg).eval()


def test_cross_encoder_matches_hf():
    hf = _hf()
    sd = hf.state_dict()
    assert float(sd["classifier.weight"].abs().max()) > 0 and float(sd["bert.pooler.dense.weight"].abs().max()) > 0
    m = CrossEncoderModel(EncoderConfig("t", "bert", 2, 64, 2, 128, 300, max_position=512, pooling="cls"),
                          dtype=torch.float32).eval()
    m.load_hf_state_dict(sd)
    g = torch.Generator().manual_seed(6)
    pairs = []
    for nq, nd in ((3, 5), (1, 1), (7, 20), (4, 2), (10, 33), (2, 9)):
        q = torch.randint(5, 300, (nq,), generator=g).tolist()
        d = torch.randint(5, 300, (nd,), generator=g).tolist()
        pairs.append(([1] + q + [2] + d + [2], [0] * (nq + 2) + [1] * (nd + 1)))
    lens = [len(i) for i, _ in pairs]
    assert len(set(lens)) == len(lens)
    L = max(lens)
    ids = torch.zeros((len(pairs), L), dtype=torch.long)
    tt = torch.zeros((len(pairs), L), dtype=torch.long)
    mask = torch.zeros((len(pairs), L), dtype=torch.long)
    for r, (i, t) in enumerate(pairs):
        ids[r, :len(i)], tt[r, :len(i)], mask[r, :len(i)] = torch.tensor(i), torch.tensor(t), 1
    with torch.no_grad():
        want = hf(input_ids=ids, token_type_ids=tt, attention_mask=mask).logits[:, 0]
    flat = torch.tensor(sum((i for i, _ in pairs), []), dtype=torch.int32)
    types = torch.tensor(sum((t for _, t in pairs), []), dtype=torch.int32)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    pos = torch.tensor(sum((list(range(n)) for n in lens), []), dtype=torch.int32)
    got = m(flat, cu, pos, lens, type_ids=types)
    assert got.dtype == torch.float32 and got.shape == (6,)
    assert torch.allclose(got, want, atol=1e-4), (got - want).abs().max()
    sig = m(flat, cu, pos, lens, type_ids=types, activation=1)
    assert torch.allclose(sig, torch.sigmoid(want), atol=1e-4)


def test_cross_encoder_rejects_two_labels():
    m = CrossEncoderModel(EncoderConfig("t", "bert", 2, 64, 2, 128, 300, max_position=512, pooling="cls"),
                          dtype=torch.float32)
    with pytest.raises(ValueError, match="num_labels"):
        m.load_hf_state_dict(_hf(2).state_dict())


def test_presets_and_random_init():
    assert set(RERANKERS) == {"ms-marco-minilm-l6", "rerank-tiny"} and not set(RERANKERS) & set(ENCODERS)
    c = RERANKERS["ms-marco-minilm-l6"]
    assert (c.arch, c.num_layers, c.hidden, c.num_heads, c.intermediate, c.vocab_size, c.max_position,
            c.type_vocab_size) == ("bert", 6, 384, 12, 1536, 30522, 512, 2)
    t, b = RERANKERS["rerank-tiny"], ENCODERS["bert-tiny"]
    assert (t.num_layers, t.hidden, t.num_heads, t.intermediate, t.vocab_size) == (
        b.num_layers, b.hidden, b.num_heads, b.intermediate, 32768)
    m = build_reranker("rerank-tiny", dtype=torch.float32)
    assert m.pool_w.shape == (128, 128) and m.cls_w.shape == (1, 128) and m.cls_b.shape == (1,)
    assert float(m.cls_w.abs().max()) > 0 and float(m.pool_w.abs().max()) > 0
    assert float(m.pool_b.abs().max()) == 0 and float(m.cls_b.abs().max()) == 0


# ------------------------------------------------------------------ tokeniser
def test_encode_pairs_layout_and_truncation():
    tok = builtin_tokenizer()
    q, docs = "how to scale a deployment", ["scale it with kubectl", "", "logs " * 400]
    ids, types = tok.encode_pairs(q, docs, 64)
    nq = len(tok.encode(q))
    for i, t in zip(ids, types):
        assert len(i) == len(t) <= 64 and i[0] == tok.cls_id and i[-1] == tok.sep_id
        first = i.index(tok.sep_id)
        assert first == nq + 1 and i.count(tok.sep_id) >= 2
        assert t == [0] * (first + 1) + [1] * (len(i) - first - 1)  # switches exactly after the first [SEP]
    assert len(ids[1]) == nq + 3 and len(ids[2]) == 64  # empty document; over-long document
    # over-long query: capped at (max_len - 3) // 2, the document fills the rest
    lq = "deployment " * 300
    ids, types = tok.encode_pairs(lq, ["short doc", "pod " * 300], 33)
    cap = (33 - 3) // 2
    for i, t in zip(ids, types):
        first = i.index(tok.sep_id)
        assert first == cap + 1 and i[1:first] == tok.encode(lq)[:cap]
        assert len(i) <= 33 and i[-1] == tok.sep_id and t[first] == 0 and t[first + 1] == 1 and t[-1] == 1
    assert len(ids[1]) == 33 and len(ids[0]) == cap + 2 + len(tok.encode("short doc")) + 1


# ------------------------------------------------------------------ routes
@pytest.fixture(scope="module")
def served():
    mgr = ModelManager(Config(), device="cpu", aliases=ALIASES)
    with TestClient(create_app(mgr)) as c:
        yield c, mgr
    mgr.shutdown()


DOCS = ["Scale the deployment with kubectl scale.", "Read the logs of the pod.", "Scale the deployment with kubectl scale.",
        {"text": "Namespaces dev and staging allow restarts."}, "queue depth"]


def _texts(docs):
    return [d["text"] if isinstance(d, dict) else d for d in docs]


def test_route_order_ties_scores_and_usage(served):
    c, mgr = served
    before = c.get("/api/tags").json()
    q = "how do I scale the deployment"
    for route in ("/v1/rerank", "/api/rerank"):
        r = c.post(route, json={"model": "rr", "query": q, "documents": DOCS})
        assert r.status_code == 200, r.text
        out = r.json()
        assert out["model"] == "rr" and sorted(x["index"] for x in out["results"]) == list(range(5))
        assert all("document" not in x for x in out["results"])
        eng = mgr.reranker("rr").engine
        logits = eng.score(q, _texts(DOCS)).double()
        assert logits.shape == (5,) and logits.dtype == torch.float64
        want = torch.sigmoid(logits).tolist()
        for x in out["results"]:
            assert abs(x["relevance_score"] - want[x["index"]]) <= 1e-6
        sc = [x["relevance_score"] for x in out["results"]]
        assert sc == sorted(sc, reverse=True) and len(set(sc)) >= 3
        # the two identical documents tie: lower index first
        pos = {x["index"]: k for k, x in enumerate(out["results"])}
        by = {x["index"]: x["relevance_score"] for x in out["results"]}
        assert by[0] == by[2] and pos[2] == pos[0] + 1
        ids, _ = eng.encode(q, _texts(DOCS))
        assert out["usage"] == {"total_tokens": sum(map(len, ids))}
    # listed once loaded, not before
    names = lambda t: [m["name"] for m in t["models"]]  # noqa: E731
    assert "rr:latest" not in names(before) and "rr:latest" in names(c.get("/api/tags").json())
    assert "rr" in [m["name"] for m in c.get("/api/ps").json()["models"]]


def test_route_top_n_return_documents_and_empty(served):
    c, mgr = served
    body = {"model": "rr", "query": "scale", "documents": DOCS}
    full = c.post("/v1/rerank", json=body).json()["results"]
    out = c.post("/v1/rerank", json={**body, "top_n": 2, "return_documents": True}).json()
    assert [x["index"] for x in out["results"]] == [x["index"] for x in full[:2]]
    assert [x["document"] for x in out["results"]] == [{"text": _texts(DOCS)[x["index"]]} for x in out["results"]]
    assert len(c.post("/v1/rerank", json={**body, "top_n": 99}).json()["results"]) == 5
    # no documents: nothing is scored (a manager with nothing loaded stays that way)
    fresh = ModelManager(Config(), device="cpu", aliases=ALIASES)
    r = TestClient(create_app(fresh)).post("/v1/rerank", json={"model": "rr", "query": "x", "documents": []})
    assert r.status_code == 200 and r.json() == {"model": "rr", "results": [], "usage": {"total_tokens": 0}}
    assert not fresh.rerankers


@pytest.mark.parametrize("patch,field", [
    ({"query": None}, "query"), ({"query": "   "}, "query"), ({"query": 3}, "query"),
    ({"documents": "a string"}, "documents"), ({"documents": None}, "documents"),
    ({"documents": ["ok", 5]}, "documents"), ({"documents": [{"text": 1}]}, "documents"),
    ({"documents": [{"body": "x"}]}, "documents"), ({"documents": ["d"] * 1025}, "documents"),
    ({"top_n": 0}, "top_n"), ({"top_n": -3}, "top_n"), ({"top_n": 1.5}, "top_n"),
])
def test_route_400s_name_the_field(served, patch, field):
    c, _ = served
    body = {"model": "rr", "query": "scale", "documents": ["a", "b"], **patch}
    body = {k: v for k, v in body.items() if v is not None}
    r = c.post("/v1/rerank", json=body)
    assert r.status_code == 400 and field in r.json()["error"], r.text


def test_route_model_errors_and_capability(served):
    c, _ = served
    r = c.post("/v1/rerank", json={"model": "no-such-model", "query": "x", "documents": ["a"]})
    assert r.status_code == 404
    r = c.post("/v1/rerank", json={"model": "emb", "query": "x", "documents": ["a"]})
    assert r.status_code == 400 and "does not support rerank" in r.json()["error"]
    r = c.post("/api/embed", json={"model": "rr", "input": ["a"]})
    assert r.status_code == 400 and "does not support embeddings" in r.json()["error"]
    assert c.post("/api/embeddings", json={"model": "rr", "prompt": "a"}).status_code == 400
    assert c.post("/api/show", json={"model": "rr"}).json()["capabilities"] == ["rerank"]
    assert c.post("/api/show", json={"model": "emb"}).json()["capabilities"] == ["embedding"]
    assert c.post("/api/show", json={"model": "ms-marco-minilm-l6"}).json()["capabilities"] == ["rerank"]
    assert c.post("/api/embed", json={"model": "emb", "input": ["a"]}).status_code == 200


def test_engine_micro_batches_and_score_cpu():
    from llm_kubernetes_minikube_sharp4dev_amd.engine.rerank_engine import RerankEngine

    m = build_reranker("rerank-tiny", dtype=torch.float32)
    whole = RerankEngine(m, builtin_tokenizer(), max_len=64)
    docs = [P.PAIR_DOCS[i % len(P.PAIR_DOCS)] + f" {i}" for i in range(20)]
    ids, _ = whole.encode(P.PAIR_QUERY, docs)
    small = RerankEngine(m, builtin_tokenizer(), max_tokens_per_batch=sum(map(len, ids)) // 3 + 1, max_len=64)
    a, b = whole.score(P.PAIR_QUERY, docs), small.score(P.PAIR_QUERY, docs)
    assert a.shape == (20,) and torch.allclose(a, b, atol=1e-5) and float(a.std()) > 0
    s, ntok = small.score_cpu(P.PAIR_QUERY, docs, 1, return_tokens=True)
    assert isinstance(s, np.ndarray) and s.dtype == np.float32 and ntok == sum(map(len, ids))
    assert np.allclose(s, torch.sigmoid(a).numpy(), atol=1e-6)
    assert whole.score(P.PAIR_QUERY, []).shape == (0,)


# ------------------------------------------------------------------ split server
def test_frontend_over_fake_core_returns_its_scores_sorted():
    from llm_kubernetes_minikube_sharp4dev_amd.serving.fake_core import FakeCore, fake_rerank_scores
    from llm_kubernetes_minikube_sharp4dev_amd.serving.remote import create_frontend_app

    path = os.path.join(tempfile.mkdtemp(), "fake.sock")
    loop = asyncio.new_event_loop()
    th = threading.Thread(target=loop.run_forever, daemon=True)
    th.start()
    core = FakeCore(path)
    asyncio.run_coroutine_threadsafe(core.start(), loop).result(10)
    try:
        fe = create_frontend_app([path], Config(), {"rerank-fake": "rerank-tiny"})
        docs = ["alpha", "beta gamma", "alpha", "delta", "epsilon zeta eta"]
        with TestClient(fe) as c:
            r = c.post("/v1/rerank", json={"model": "rerank-fake", "query": "which letter", "documents": docs, "top_n": 4})
            assert r.status_code == 200, r.text
            out = r.json()
            want = fake_rerank_scores("which letter", docs, 1)
            order = sorted(range(5), key=lambda i: (-float(want[i]), i))[:4]
            assert [x["index"] for x in out["results"]] == order
            assert [x["relevance_score"] for x in out["results"]] == [float(want[i]) for i in order]
            assert order.index(2) == order.index(0) + 1
            assert out["usage"]["total_tokens"] == sum(2 + len(d.split()) + 3 for d in docs)
            assert c.post("/v1/rerank", json={"model": "rerank-fake", "query": "q", "documents": []}).json()["results"] == []
    finally:
        loop.call_soon_threadsafe(core._server.close)
        loop.call_soon_threadsafe(loop.stop)
        th.join(5)


def test_real_core_rerank_matches_in_process():
    """The engine core's rerank op (on the embed op's pool) against the in-process route."""
    from llm_kubernetes_minikube_sharp4dev_amd.serving.engine_core import EngineCore
    from llm_kubernetes_minikube_sharp4dev_amd.serving.remote import create_frontend_app

    d = tempfile.mkdtemp()
    m = ModelManager(Config(), device="cpu", aliases=ALIASES)
    core = EngineCore(m, os.path.join(d, "core.sock"))
    local = ModelManager(Config(), device="cpu", aliases=ALIASES)
    try:
        fe = create_frontend_app([core.path], Config(), ALIASES, preload=["rr"])
        body = {"model": "rr", "query": "scale the deployment", "documents": DOCS, "return_documents": True}
        with TestClient(fe) as c_fe, TestClient(create_app(local)) as c_local:
            a, b = c_fe.post("/v1/rerank", json=body), c_local.post("/v1/rerank", json=body)
            assert a.status_code == b.status_code == 200 and a.json() == b.json()
            r = c_fe.post("/v1/rerank", json={**body, "model": "emb"})
            assert r.status_code == 400
    finally:
        core.close()
        m.shutdown()
        local.shutdown()


# ------------------------------------------------------------------ /rag/search
class _Reverse:
    """Scripted reranker: the later a document arrives (the lower its cosine), the higher its score."""

    def __init__(self):
        self.calls = []

    def score(self, query, docs):
        self.calls.append((query, list(docs)))
        return [float(i) for i in range(len(docs))]


def _index(n=40):
    from llm_kubernetes_minikube_sharp4dev_amd.rag.embedder import HashEmbedder
    from llm_kubernetes_minikube_sharp4dev_amd.rag.index import RagIndex

    emb = HashEmbedder(128)
    idx = RagIndex(emb, backend="exact")
    # every chunk shares the query's words; chunk i carries i words of noise, so the cosines
    # fall slowly and the 24 candidates all stay above the 0.20 floor
    noise = [f"w{j}x" for j in range(n)]
    texts = ["scale deployment replicas queue scale deployment replicas queue " + " ".join(noise[:i]) + f" s{i}"
             for i in range(n)]
    idx.add([f"c{i}" for i in range(n)], [f"doc{i % 4}.md" for i in range(n)], texts, emb.embed(texts))
    return idx


def test_rag_query_reranks_the_candidates():
    idx = _index()
    q = "scale deployment replicas queue"
    cos = idx.query(q, 24)
    assert len(cos) == 24 and all(h.rerank_score is None for h in cos)
    rr = _Reverse()
    got = idx.query(q, 5, reranker=rr, candidates=24)
    assert rr.calls == [(q, [h.text for h in cos])]
    assert [h.id for h in got] == [h.id for h in cos[::-1][:5]]
    assert [h.score for h in got] == [h.score for h in cos[::-1][:5]]  # still the cosine
    assert [h.rerank_score for h in got] == [23.0, 22.0, 21.0, 20.0, 19.0]
    assert [h.id for h in idx.query(q, 5)] == [h.id for h in cos[:5]]


def test_rag_search_route_opt_in_and_unchanged_without():
    from llm_kubernetes_minikube_sharp4dev_amd.apps.rag_app import create_rag_app

    idx = _index()
    body = {"query": "scale deployment replicas queue", "topK": 4}
    plain = TestClient(create_rag_app(Config(), idx, build_index=False)).post("/rag/search", json=body)
    # without rerank_model a reranker that is handed in is not used: byte-identical JSON
    rr = _Reverse()
    same = TestClient(create_rag_app(Config(), idx, build_index=False, reranker=rr)).post("/rag/search", json=body)
    assert plain.status_code == 200 and same.text == plain.text and not rr.calls and "rerankScore" not in plain.text
    cos = idx.query(body["query"], 24)
    assert min(h.score for h in cos) >= 0.20
    want_plain = [{"id": h.id, "source": h.source, "score": h.score} for h in cos[:4]]
    assert [{k: x[k] for k in ("id", "source", "score")} for x in plain.json()] == want_plain
    assert all(list(x) == ["id", "source", "score", "preview"] for x in plain.json())
    cfg = Config()
    cfg.rag.rerank_model = "rr"
    assert cfg.rag.rerank_candidates == 24 and Config().rag.rerank_model is None
    out = TestClient(create_rag_app(cfg, idx, build_index=False, reranker=rr)).post("/rag/search", json=body).json()
    assert [x["id"] for x in out] == [h.id for h in cos[::-1][:4]]
    assert [x["score"] for x in out] == [h.score for h in cos[::-1][:4]]
    assert [x["rerankScore"] for x in out] == [23.0, 22.0, 21.0, 20.0] and all("preview" in x for x in out)
    with pytest.raises(ValueError, match="rerank_model"):
        create_rag_app(cfg, idx, build_index=False)
