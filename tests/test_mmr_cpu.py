"""MMR as the last retrieval stage without a GPU: RagIndex.query / search_vectors on a small HashEmbedder
index against a hand computation, the relevance maps (lam = 1 keeps every mode's order), the
``mmrLambda`` switch of POST /rag/search, the sharded refusals, /agent_rag's two retrieval paths and the
settings."""
import json

import numpy as np
import pytest
import torch
from fastapi.testclient import TestClient

from llm_kubernetes_minikube_sharp4dev_amd.apps.common import NetJSONResponse
from llm_kubernetes_minikube_sharp4dev_amd.config import Config, RagConfig, load_config
from llm_kubernetes_minikube_sharp4dev_amd.rag.embedder import HashEmbedder
from llm_kubernetes_minikube_sharp4dev_amd.rag.index import RagIndex, cosine_exact, mmr_select_f64

IDENT = "ErrImageNeverPull"
COPY = "alpha beta gamma delta epsilon"
QUERY = "alpha beta gamma delta"


def _index(n=40, at=17, backend="exact", device=None):
    emb = HashEmbedder(128)
    idx = RagIndex(emb, backend=backend, device=device)
    noise = [f"w{j}x" for j in range(n)]
    texts = ["scale deployment replicas queue scale deployment replicas queue " + " ".join(noise[:i]) + f" s{i}"
             for i in range(n)]
    texts[at] += f" the pod stays in {IDENT}"
    idx.add([f"c{i}" for i in range(n)], [f"doc{i % 4}.md" for i in range(n)], texts, emb.embed(texts))
    return idx


def _copies_index(backend="exact", device=None):
    """Four copies of one chunk (ids k0..k3, the best hits of QUERY), eight distinct chunks that share
    three of its five words, and filler."""
    emb = HashEmbedder(128)
    idx = RagIndex(emb, backend=backend, device=device)
    texts, ids = [], []
    for i in range(8):
        texts.append(f"alpha beta gamma zeta{i}q")
        ids.append(f"d{i}")
    for i in range(4):
        texts.insert(2 * i + 1, COPY)
        ids.insert(2 * i + 1, f"k{i}")
    for i in range(12):
        texts.append(f"omega{i}a sigma{i}b alpha tau{i}c")
        ids.append(f"f{i}")
    idx.add(ids, ["runbook.md"] * len(ids), texts, emb.embed(texts))
    return idx


class Reverse:
    """A stub reranker: the later a document comes, the better."""

    def score(self, query, docs):
        return [float(i) for i in range(len(docs))]


# ------------------------------------------------------------------ RagIndex
def test_hand_computed_example():
    idx = _index()
    q = "scale deployment " + IDENT
    k, pool, lam = 5, 24, 0.5
    cand = idx.query(q, pool)
    rank = {c.id: i for i, c in enumerate(idx.chunks)}
    rows = idx.matrix()[[rank[h.id] for h in cand]]
    rel = [h.score for h in cand]
    # by hand, in float64: the greedy rounds of docs/mmr.md
    sel, m, want = [], [0.0] * pool, []
    for r in range(k):
        v = [lam * rel[i] - (1 - lam) * m[i] for i in range(pool)]
        p = min((i for i in range(pool) if i not in sel), key=lambda i: (-v[i], i))
        want.append((cand[p].id, v[p], m[p]))
        sel.append(p)
        sim = [cosine_exact(rows[i], rows[p]) for i in range(pool)]
        m = sim if r == 0 else [max(a, b) for a, b in zip(m, sim)]
    got = idx.query(q, k, mmr_lambda=lam, mmr_candidates=pool)
    assert [h.id for h in got] == [w[0] for w in want]
    assert [h.mmr_score for h in got] == pytest.approx([w[1] for w in want], abs=1e-12)
    assert [h.max_sim for h in got] == pytest.approx([w[2] for w in want], abs=1e-12)
    assert got[0].id == cand[0].id and got[0].max_sim == 0.0 and got[0].mmr_score == lam * cand[0].score
    assert [h.id for h in got] != [h.id for h in cand[:k]]             # the near-copies of c0 moved back
    assert all(h.score == rel[[c.id for c in cand].index(h.id)] for h in got)     # `score` stays the cosine
    # the pool: min(64, max(top_k, mmr_candidates)) hits
    assert [h.id for h in idx.query(q, 3, mmr_lambda=lam, mmr_candidates=2)] == [
        cand[p].id for p, _, _ in mmr_select_f64(rows[:3], rel[:3], lam, 3)]
    assert sorted(h.id for h in idx.query(q, 3, mmr_lambda=lam, mmr_candidates=2)) == sorted(h.id for h in cand[:3])
    assert len(idx.query(q, 40, mmr_lambda=lam, mmr_candidates=500)) == 40
    # None is the path without the stage
    assert [(h.id, h.score, h.mmr_score, h.max_sim) for h in idx.query(q, k, mmr_lambda=None)] == [
        (h.id, h.score, None, None) for h in cand[:k]]
    for bad in (1.5, -0.1, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="mmr_lambda"):
            idx.query(q, k, mmr_lambda=bad)
    assert RagIndex(HashEmbedder(128), backend="exact").query(q, k, mmr_lambda=0.5) == []


def test_planted_copies_leave_the_result():
    for backend, dev in (("exact", None), ("gpu", "cpu")):  # 'gpu' on the CPU: ops.mmr_select's fp32 reference
        idx = _copies_index(backend, dev)
        assert [h.id for h in idx.query(QUERY, 4)] == ["k0", "k1", "k2", "k3"]
        got = idx.query(QUERY, 6, mmr_lambda=0.5)
        assert got[0].id == "k0" and not any(h.id.startswith("k") for h in got[1:]), [h.id for h in got]
        assert sum(h.id.startswith("d") for h in got) >= 4
        rows = idx.search_vectors(idx.embedder.embed([QUERY]), 6, mmr=(0.5, 24))[0]
        assert [idx.chunks[j].id for j, _ in rows] == [h.id for h in got]
        assert [s for _, s in rows] == pytest.approx([h.score for h in got], abs=1e-6)
        assert idx.search_vectors_async(idx.embedder.embed([QUERY]), 6, mmr=(0.5, 24)).result() == [rows]


@pytest.mark.parametrize("mode", ["dense", "lexical", "hybrid"])
def test_lambda_one_keeps_the_order_and_lambda_zero_the_top_hit(mode):
    idx = _index()
    for q in (IDENT, "scale deployment replicas " + IDENT, "queue w3x w5x"):
        for rr in (None, Reverse()):
            want = idx.query(q, 6, reranker=rr, candidates=24, mode=mode)
            got = idx.query(q, 6, reranker=rr, candidates=24, mode=mode, mmr_lambda=1.0)
            assert [h.id for h in got] == [h.id for h in want]
            assert [(h.score, h.rerank_score, h.lexical_score, h.fused_score) for h in got] == [
                (h.score, h.rerank_score, h.lexical_score, h.fused_score) for h in want]
            if got:
                # the relevance of each mode, as lam = 1 reports it
                rel = ([h.rerank_score for h in want] if rr else [h.score for h in want] if mode == "dense" else
                       [h.fused_score * 61 / (2 if mode == "hybrid" else 1) for h in want])
                assert [h.mmr_score for h in got] == pytest.approx(rel, abs=1e-12)
                assert mode == "dense" or rr or all(0 < x <= 1 for x in rel)
                zero = idx.query(q, 6, reranker=rr, candidates=24, mode=mode, mmr_lambda=0.0)
                assert zero[0].id == want[0].id and len(zero) == len(want)


def test_sharded_corpus_refuses_mmr():
    idx = _index()
    qv = idx.embedder.embed([IDENT])
    idx.set_sharded(lambda q, k: (_ for _ in ()).throw(AssertionError("not reached")), dim=128)
    with pytest.raises(ValueError, match="sharded"):
        idx.query(IDENT, 5, mmr_lambda=0.5)
    with pytest.raises(ValueError, match="sharded"):
        idx.search_vectors(qv, 5, mmr=(0.5, 24))
    with pytest.raises(ValueError, match="sharded"):
        idx.search_vectors_async(qv, 5, mmr=(0.5, 24))


def test_mmr_span():
    from llm_kubernetes_minikube_sharp4dev_amd.utils import tracing

    idx = _index()
    idx.query(IDENT, 3, mmr_lambda=0.25, mmr_candidates=9)
    spans = [r for r in tracing.recent(20) if r["span"] == "rag.mmr"]
    assert spans and spans[-1]["component"] == "rag_index" and spans[-1]["lam"] == 0.25 and spans[-1]["candidates"] == 9


# ------------------------------------------------------------------ /rag/search
def _body(hits, preview_chars=260):
    rows = []
    for h in hits:
        row = {"id": h.id, "source": h.source, "score": h.score}
        if h.fused_score is not None:
            row.update(lexicalScore=h.lexical_score, fusedScore=h.fused_score)
        if h.rerank_score is not None:
            row["rerankScore"] = h.rerank_score
        row["preview"] = h.text[:preview_chars] + "..." if len(h.text) > preview_chars else h.text
        rows.append(row)
    return NetJSONResponse(rows).body


def test_rag_search_mmr_lambda():
    from llm_kubernetes_minikube_sharp4dev_amd.apps.rag_app import create_rag_app

    idx = _index()
    q = "scale deployment " + IDENT
    c = TestClient(create_rag_app(Config(), idx, build_index=False))
    body = {"query": q, "topK": 4}
    # without MMR: byte for byte the body made from index.query as it was before the stage
    for mode in ("dense", "lexical", "hybrid"):
        want = _body(idx.query(q, 4, mode=mode))
        assert c.post("/rag/search", json={**body, "mode": mode}).content == want
        assert c.post("/rag/search", json={**body, "mode": mode, "mmrLambda": None}).content == want
    assert b"mmrScore" not in c.post("/rag/search", json=body).content
    # with it
    for lam in (0, 1, 0.5, 0.25):
        want = idx.query(q, 4, mmr_lambda=lam)
        out = c.post("/rag/search", json={**body, "mmrLambda": lam})
        assert out.status_code == 200
        rows = out.json()
        assert all(list(x) == ["id", "source", "score", "mmrScore", "maxSim", "preview"] for x in rows)
        assert [(x["id"], x["score"], x["mmrScore"], x["maxSim"]) for x in rows] == [
            (h.id, h.score, h.mmr_score, h.max_sim) for h in want]
    assert [x["id"] for x in c.post("/rag/search", json={**body, "mmrLambda": 1}).json()] == [
        x["id"] for x in c.post("/rag/search", json=body).json()]
    half = c.post("/rag/search", json={**body, "mmrLambda": 0.5})
    for key in ("MMRLAMBDA", "mmrlambda", "MmrLambda"):
        assert c.post("/rag/search", json={**body, key: 0.5}).content == half.content
    hyb = c.post("/rag/search", json={**body, "mode": "hybrid", "mmrLambda": 0.5}).json()
    assert all(list(x) == ["id", "source", "score", "lexicalScore", "fusedScore", "mmrScore", "maxSim", "preview"] for x in hyb)
    assert [x["id"] for x in hyb] == [h.id for h in idx.query(q, 4, mode="hybrid", mmr_lambda=0.5)]
    for bad in ("0.5", True, False, 1.5, -0.1, [0.5], {"v": 1}):
        r = c.post("/rag/search", json={**body, "mmrLambda": bad})
        assert r.status_code == 400 and r.json() == {"error": "mmrLambda must be a number between 0 and 1"}, r.text
    r = c.post("/rag/search", content=json.dumps(body)[:-1] + ', "mmrLambda": NaN}', headers={"content-type": "application/json"})
    assert r.status_code == 400 and r.json() == {"error": "mmrLambda must be a number between 0 and 1"}
    # with a reranker the extra fields follow rerankScore
    cfg = Config()
    cfg.rag.rerank_model = "stub"
    cr = TestClient(create_rag_app(cfg, idx, build_index=False, reranker=Reverse()))
    assert cr.post("/rag/search", json=body).content == _body(idx.query(q, 4, reranker=Reverse(), candidates=24))
    rows = cr.post("/rag/search", json={**body, "mmrLambda": 0.5}).json()
    assert all(list(x) == ["id", "source", "score", "rerankScore", "mmrScore", "maxSim", "preview"] for x in rows)
    assert [x["id"] for x in rows] == [h.id for h in idx.query(q, 4, reranker=Reverse(), candidates=24, mmr_lambda=0.5)]
    # the configured default, and null to switch it off for one request
    cfg = Config()
    cfg.rag.mmr_lambda, cfg.rag.mmr_candidates = 0.5, 12
    c2 = TestClient(create_rag_app(cfg, idx, build_index=False))
    assert [x["id"] for x in c2.post("/rag/search", json=body).json()] == [
        h.id for h in idx.query(q, 4, mmr_lambda=0.5, mmr_candidates=12)]
    assert c2.post("/rag/search", json={**body, "mmrLambda": None}).content == c.post("/rag/search", json=body).content
    assert c2.post("/rag/search", json={**body, "mmrLambda": 1}).json()[1]["mmrScore"] is not None
    # a sharded corpus answers MMR with a 400 that carries the ValueError's message
    idx.set_sharded(lambda qv, k: (torch.zeros(len(qv), k), torch.zeros(len(qv), k, dtype=torch.int32)), dim=128)
    r = c.post("/rag/search", json={**body, "mmrLambda": 0.5})
    assert r.status_code == 400 and "sharded" in r.json()["error"] and "MMR" in r.json()["error"]
    with pytest.raises(ValueError) as e:
        idx.query(q, 4, mmr_lambda=0.5)
    assert r.json()["error"] == str(e.value)


# ------------------------------------------------------------------ /agent_rag
class Tok:
    def chat_prompt_batch(self, texts, style=None):
        return [[1, 2, 3] for _ in texts]


def test_agent_pipeline_plan_with_and_without_agent_mmr_lambda():
    from llm_kubernetes_minikube_sharp4dev_amd.agent.rag_pipeline import RagAgentPipeline

    idx = _copies_index()
    cfg = Config()
    pipe = RagAgentPipeline(idx, None, Tok(), None, cfg)
    (plan,), _ = pipe.plan([QUERY])
    today = [h.id for h in plan[3]]
    assert today[:4] == ["k0", "k1", "k2", "k3"] and plan[2] == today          # four copies in the evidence
    # exactly what the pipeline made of search_vectors(q, agent_topk) before
    hits = idx.hits(idx.search_vectors(idx.embedder.embed([QUERY]), cfg.rag.agent_topk)[0])
    best = max(h.score for h in hits)
    assert today == [h.id for h in hits if h.score >= max(cfg.rag.evidence_min_score, best * cfg.rag.citation_best_ratio)]
    cfg2 = Config()
    cfg2.rag.agent_mmr_lambda = 0.5
    (plan2,), _ = RagAgentPipeline(idx, None, Tok(), None, cfg2).plan([QUERY])
    ev = [h.id for h in plan2[3]]
    assert ev[0] == "k0" and sum(i.startswith("k") for i in ev) == 1 and sum(i.startswith("d") for i in ev) >= 4, ev
    assert plan2[1] == [1, 2, 3] and plan2[0] == QUERY
    assert plan2[3][0].score == plan[3][0].score                               # `best` is the same hit


def test_agent_rag_route_uses_agent_mmr_lambda():
    from llm_kubernetes_minikube_sharp4dev_amd.apps.rag_app import create_rag_app

    class LLM:
        def __init__(self):
            self.prompts = []

        async def generate(self, prompt):
            self.prompts.append(prompt)
            return "{}"

    idx = _copies_index()
    seen = {}
    for lam in (None, 0.5):
        cfg = Config()
        cfg.rag.agent_mmr_lambda = lam
        llm = LLM()
        with TestClient(create_rag_app(cfg, idx, llm=llm, build_index=False)) as c:
            c.post("/agent_rag", json={"prompt": QUERY})
        assert len(llm.prompts) == 1
        seen[lam] = llm.prompts[0].count("epsilon")                            # a word of the copies only
    assert seen == {None: 4, 0.5: 1}


# ------------------------------------------------------------------ settings
def test_settings_defaults_overrides_and_validation():
    from llm_kubernetes_minikube_sharp4dev_amd.apps.rag_app import create_rag_app

    r = RagConfig()
    assert (r.mmr_lambda, r.mmr_candidates, r.agent_mmr_lambda) == (None, 24, None)
    c = load_config(env={"LK_RAG__MMR_LAMBDA": "0.5", "LK_RAG__AGENT_MMR_LAMBDA": "1"}, cli={"rag.mmr_candidates": "32"})
    assert (c.rag.mmr_lambda, c.rag.mmr_candidates, c.rag.agent_mmr_lambda) == (0.5, 32, 1)
    idx = _index()
    create_rag_app(c, idx, build_index=False)
    for name, bad in (("mmr_lambda", 1.5), ("mmr_lambda", "x"), ("agent_mmr_lambda", -1), ("agent_mmr_lambda", True),
                      ("mmr_lambda", float("nan")), ("mmr_candidates", 0), ("mmr_candidates", 2.5)):
        cfg = Config()
        setattr(cfg.rag, name, bad)
        with pytest.raises(ValueError, match=f"rag.{name}"):
            create_rag_app(cfg, idx, build_index=False)
