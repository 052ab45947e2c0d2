"""Hybrid retrieval without a GPU: the BM25 reference on the exact probes, the analyser, the
lexical index's invariants, reciprocal-rank fusion in RagIndex.query against a hand-computed
example, and the ``mode`` switch of POST /rag/search."""
from collections import Counter

import numpy as np
import pytest
import torch
from fastapi.testclient import TestClient

import bm25_probes as P
from llm_kubernetes_minikube_sharp4dev_amd import ops
from llm_kubernetes_minikube_sharp4dev_amd.config import Config, RagConfig
from llm_kubernetes_minikube_sharp4dev_amd.rag.embedder import HashEmbedder
from llm_kubernetes_minikube_sharp4dev_amd.rag.index import RagIndex
from llm_kubernetes_minikube_sharp4dev_amd.rag.lexical import LexicalIndex, analyse, split_run

C = ops.reference.BM25_CHUNK


# ------------------------------------------------------------------ the reference on the exact probes
@pytest.mark.parametrize("tf255", [False, True])
@pytest.mark.parametrize("N", [1, C - 1, C, C + 1, 3 * C + 5])
def test_reference_exact_probes(N, tf255):
    for nq in (1, 3, 33):
        for K in (1, 5, 64):
            p = P.exact_probe(N, nq, K, tf255)
            for fn in (ops.bm25_topk, ops.reference.bm25_topk):
                s, i = fn(*P.probe_args(p), K)
                P.check_exact(s, i, p, (N, nq, K, tf255))


def test_probe_patterns_are_present():
    p = P.exact_probe(3 * C + 5, 33, 64)
    tp, qp = p["term_ptr"].numpy(), p["q_ptr"].numpy()
    df = np.diff(tp)
    assert df[0] == 3 * C + 5 and df[1] == 1 and df[2] == 1 and df[3] == 0
    assert p["post_doc"][tp[1]] == 0 and p["post_doc"][tp[2]] == 3 * C + 4
    lens = np.diff(qp)
    assert lens[0] == 64 and lens[1] == 0 and lens.max() == 64
    assert np.all(p["exp_i"][1] == -1) and np.all(np.isinf(p["exp_s"][1]))       # no terms: all pads
    assert p["exp_i"][2].tolist()[:3] == [0, 3 * C + 4, -1]                         # fewer hits than K
    assert np.all(p["exp_i"][4] == -1)                                              # an empty posting list
    s3, i3 = p["exp_s"][3], p["exp_i"][3]                                           # df = N alone: ties
    tie = np.flatnonzero(np.diff(s3) == 0)
    assert len(tie) and np.all(np.diff(i3)[tie] > 0)
    # equal scores across chunks (the index has period 64 in the document id): the best score of
    # the 64-term query belongs to one document in 64, in every chunk alike -- each chunk offers 64
    # candidates of that score and the 64 lowest ids, all in chunk 0, have to win the merge
    s0, i0 = p["exp_s"][0], p["exp_i"][0]
    assert s0[0] == s0[-1] and i0[0] < 64 and np.array_equal(i0, i0[0] + 64 * np.arange(64))


def test_reference_refusals_and_random_bound():
    p = P.exact_probe(C + 1, 3, 5)
    a = P.probe_args(p)
    with pytest.raises(ValueError, match="K must be in"):
        ops.bm25_topk(*a, 65)
    with pytest.raises(ValueError, match="q_ptr"):
        ops.bm25_topk(*a[:4], a[4][:-1].clone(), a[5], a[6], 5)
    qp = torch.tensor([0, 65], dtype=torch.int32)
    with pytest.raises(ValueError, match="more than 64 terms"):
        ops.bm25_topk(*a[:4], qp, torch.arange(65, dtype=torch.int32), torch.ones(65), 5)
    r = P.random_index(3 * C + 5)
    s, i = ops.reference.bm25_topk(*P.probe_args(r), 10)
    err, bound, ratio = P.check_within_bound(s, i, r, 10)
    assert 0 < ratio <= 1


# ------------------------------------------------------------------ the analyser
def test_analyser_cases():
    assert analyse("CrashLoopBackOff") == ["crashloopbackoff", "crash", "loop", "back", "off"]
    assert analyse("HTTPServer") == ["httpserver", "http", "server"]
    assert split_run("HTTPServer") == ["HTTP", "Server"]
    # letter<->digit cuts give one-character parts here: only the runs themselves are terms
    assert analyse("nginx-7d9c") == ["nginx", "7d9c"]
    assert analyse("exit code 137, OOMKilled") == ["exit", "code", "137", "oomkilled", "oom", "killed"]
    assert analyse("pod2node") == ["pod2node", "pod", "node"]
    assert analyse("Perché la città È giù?") == ["perché", "la", "città", "è", "giù"]
    assert analyse("verificheràSubito") == ["verificheràsubito", "verificherà", "subito"]
    assert analyse("a" * 65 + " ok " + "b" * 64) == ["ok", "b" * 64]
    assert analyse("Ab" * 33) == []                      # a 66-character run is dropped, parts included
    assert analyse("snake_case __init__ --flag=x") == ["snake", "case", "init", "flag", "x"]
    assert analyse("") == [] and analyse("... --- ___") == []
    # a query in plain words matches the identifier's parts
    assert set(analyse("crash loop")) <= set(analyse("pod in CrashLoopBackOff"))


# ------------------------------------------------------------------ index invariants
TEXTS = ["il pod va in CrashLoopBackOff dopo il deploy", "kubectl logs del pod pod pod", "",
         "ImagePullBackOff: immagine nginx-7d9c non trovata", "pod " * 300, "HTTPServer su nodo2 risponde 503"]


def test_index_invariants():
    lex = LexicalIndex(TEXTS, k1=1.2, b=0.75)
    tp, pd, tf = lex.term_ptr.numpy(), lex.post_doc.numpy(), lex.post_tf.numpy()
    assert lex.terms == sorted(set(t for x in TEXTS for t in analyse(x))) and lex.V == len(lex.terms)
    assert tp.dtype == np.int64 and pd.dtype == np.int32 and tf.dtype == np.uint8 and lex.kn.dtype == torch.float32
    assert tp[0] == 0 and tp[-1] == len(pd) == len(tf) == lex.nnz and np.all(np.diff(tp) >= 1)
    for t in range(lex.V):
        assert np.all(np.diff(pd[tp[t]:tp[t + 1]]) > 0)  # ascending, duplicate-free
    # sum of tf per document (before the clamp) is the document's length
    counts = [Counter(analyse(x)) for x in TEXTS]
    assert lex.dl.tolist() == [sum(c.values()) for c in counts] == [len(analyse(x)) for x in TEXTS]
    pod = lex.term_id["pod"]
    docs = pd[tp[pod]:tp[pod + 1]].tolist()
    assert docs == [0, 1, 4] and tf[tp[pod]:tp[pod + 1]].tolist() == [1, 3, 255] and counts[4]["pod"] == 300
    unclamped = np.zeros(len(TEXTS), dtype=np.int64)
    for t in range(lex.V):
        for d, f in zip(pd[tp[t]:tp[t + 1]], tf[tp[t]:tp[t + 1]]):
            unclamped[d] += counts[d][lex.terms[t]]
            assert f == min(255, counts[d][lex.terms[t]])
    assert unclamped.tolist() == lex.dl.tolist()
    want_kn = 1.2 * (1 - 0.75 + 0.75 * lex.dl / lex.dl.mean())
    assert np.array_equal(lex.kn.numpy(), want_kn.astype(np.float32))
    # ids do not depend on the insertion order
    perm = [3, 5, 0, 4, 2, 1]
    other = LexicalIndex([TEXTS[i] for i in perm])
    assert other.terms == lex.terms and other.term_id == lex.term_id
    assert np.array_equal(other.df, lex.df)


def test_query_encoding():
    lex = LexicalIndex(TEXTS)
    t, w = lex.encode_one("pod pod sconosciuto CrashLoopBackOff")
    assert t == sorted(t) and set(t) == {lex.term_id[x] for x in ("pod", "crashloopbackoff", "crash", "loop", "back", "off")}
    N, df = len(TEXTS), 3
    assert w[t.index(lex.term_id["pod"])] == 2 * np.log(1 + (N - df + 0.5) / (df + 0.5))
    qp, qt, qw = lex.encode(["pod", "zzz", "crash loop"])
    assert qp.tolist() == [0, 1, 1, 3] and qp.dtype == torch.int32 and qt.dtype == torch.int32 and qw.dtype == torch.float32
    # more than 64 known terms: the 64 heaviest stay (ties to the lower id), ascending
    words = ["term" + chr(97 + i // 26) + chr(97 + i % 26) for i in range(80)]
    many = LexicalIndex(words + [words[0] + " " + words[1]])
    t, w = many.encode_one(" ".join(words))
    assert len(t) == 64 and t == sorted(t) and many.term_id[words[0]] not in t and many.term_id[words[1]] not in t
    assert t == [many.term_id[x] for x in words[2:66]]
    assert lex.search(["zzz"], 5) == [[]] and [d for d, _ in lex.search(["nginx"], 5)[0]] == [3]


# ------------------------------------------------------------------ fusion
IDENT = "ErrImageNeverPull"


def _index(n=40, at=17, backend="exact", device=None):
    emb = HashEmbedder(128)
    idx = RagIndex(emb, backend=backend, device=device)
    noise = [f"w{j}x" for j in range(n)]
    texts = ["scale deployment replicas queue scale deployment replicas queue " + " ".join(noise[:i]) + f" s{i}"
             for i in range(n)]
    texts[at] += f" the pod stays in {IDENT}"
    idx.add([f"c{i}" for i in range(n)], [f"doc{i % 4}.md" for i in range(n)], texts, emb.embed(texts))
    return idx


def test_rrf_against_hand_computed_example():
    idx = _index()
    lex = idx.query(IDENT, 5, mode="lexical")
    assert [h.id for h in lex] == ["c17"]
    assert lex[0].lexical_score > 0 and lex[0].fused_score == 1 / 61
    hyb = idx.query(IDENT, 5, mode="hybrid")
    assert len(hyb) == 5 and "c17" in [h.id for h in hyb[:2]]
    hit = next(h for h in hyb if h.id == "c17")
    assert hit.fused_score >= 1 / 61 and hit.lexical_score == lex[0].lexical_score
    # by hand: the dense list alone gives 1 / (60 + rank); c17 adds 1 / 61 from the lexical list
    dense = idx.query(IDENT, 24)
    rank = {h.id: r for r, h in enumerate(dense, 1)}
    fused = {h.id: 1 / (60 + rank[h.id]) for h in dense}
    fused["c17"] = fused.get("c17", 0.0) + 1 / 61
    num = lambda i: int(i[1:])  # noqa: E731
    want = sorted(fused, key=lambda i: (-fused[i], num(i)))[:5]
    assert [h.id for h in hyb] == want and [h.fused_score for h in hyb] == [fused[i] for i in want]
    assert all(h.lexical_score is None for h in hyb if h.id != "c17")
    # every hit keeps its cosine as `score`
    cos = {h.id: h.score for h in idx.query(IDENT, 40)}
    assert all(h.score == pytest.approx(cos[h.id], abs=1e-12) for h in hyb + lex)
    # dense is untouched, and is the default
    assert [(h.id, h.score, h.lexical_score, h.fused_score) for h in idx.query(IDENT, 5, mode="dense")] == [
        (h.id, h.score, None, None) for h in dense[:5]] == [(h.id, h.score, None, None) for h in idx.query(IDENT, 5)]
    with pytest.raises(ValueError, match="mode"):
        idx.query(IDENT, 5, mode="x")


def test_lexical_only_hit_gets_the_scan_s_cosine():
    # a query whose cosine list (2 candidates) cannot hold the identifier chunk
    idx = _index()
    idx.configure_lexical(hybrid_candidates=2)
    q = "scale deployment replicas queue " + IDENT
    dense_all = {h.id: h.score for h in idx.query(q, 40)}
    hyb = idx.query(q, 2, mode="hybrid")
    lex_ids = [h.id for h in idx.query(q, 2, mode="lexical")]
    assert lex_ids[0] == "c17"
    for h in hyb:
        assert h.score == pytest.approx(dense_all[h.id], abs=1e-12)
    # the gpu backend's formula on the host (bf16 rows, fp32 dot), against the bf16 scan's scores
    g = _index(backend="gpu", device="cpu")
    scan = dict(g.search_vectors(g.embedder.embed([q]), 40)[0])
    got = g.cosines(g.embedder.embed([q])[0], [17, 3, 39])
    assert got == pytest.approx([scan[17], scan[3], scan[39]], abs=2e-6)


def test_empty_lexical_list_and_reranker_and_invalidation():
    idx = _index()
    dense = idx.query("zzzz qqqq", 5)
    hyb = idx.query("zzzz qqqq", 5, mode="hybrid")
    assert [h.id for h in hyb] == [h.id for h in dense] and all(h.lexical_score is None for h in hyb)
    assert [h.fused_score for h in hyb] == [1 / (60 + r) for r in range(1, 6)]
    assert idx.query("zzzz qqqq", 5, mode="lexical") == []

    class Reverse:
        def __init__(self):
            self.calls = []

        def score(self, query, docs):
            self.calls.append(list(docs))
            return [float(i) for i in range(len(docs))]

    rr = Reverse()
    fused24 = idx.query(IDENT, 24, mode="hybrid")
    got = idx.query(IDENT, 3, reranker=rr, candidates=24, mode="hybrid")
    assert rr.calls == [[h.text for h in fused24]]
    assert [h.id for h in got] == [h.id for h in fused24[::-1][:3]] and [h.rerank_score for h in got] == [23.0, 22.0, 21.0]
    assert all(h.fused_score is not None for h in got)
    # add() drops the lexical index; the next query sees the new chunk
    first = idx.lexical()
    emb = idx.embedder
    idx.add(["new"], ["doc9.md"], ["a second chunk with " + IDENT], emb.embed(["a second chunk with " + IDENT]))
    assert idx.lexical() is not first and idx.lexical().N == 41
    assert sorted(h.id for h in idx.query(IDENT, 5, mode="lexical")) == ["c17", "new"]


def test_sharded_index_refuses_non_dense():
    idx = _index()
    idx.set_sharded(lambda q, k: (_ for _ in ()).throw(AssertionError("not reached")), dim=128)
    for mode in ("hybrid", "lexical"):
        with pytest.raises(ValueError, match="sharded"):
            idx.query(IDENT, 5, mode=mode)


def test_lexical_index_not_persisted_and_rebuilt_after_load(tmp_path):
    idx = _index()
    idx.lexical()
    idx.save(str(tmp_path))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["embeddings.safetensors", "index.json"]
    back = RagIndex(HashEmbedder(128), backend="exact")
    assert back.load(str(tmp_path)) and back._lex is None
    assert [h.id for h in back.query(IDENT, 5, mode="lexical")] == ["c17"]


# ------------------------------------------------------------------ /rag/search
def test_rag_search_mode():
    from llm_kubernetes_minikube_sharp4dev_amd.apps.rag_app import create_rag_app

    idx = _index()
    q = IDENT
    c = TestClient(create_rag_app(Config(), idx, build_index=False))
    body = {"query": q, "topK": 4}
    plain = c.post("/rag/search", json=body)
    assert plain.status_code == 200 and all(list(x) == ["id", "source", "score", "preview"] for x in plain.json())
    assert "lexicalScore" not in plain.text and "fusedScore" not in plain.text
    assert c.post("/rag/search", json={**body, "mode": "dense"}).text == plain.text
    want = idx.query(q, 4, mode="hybrid")
    out = c.post("/rag/search", json={**body, "mode": "hybrid"})
    assert out.status_code == 200
    rows = out.json()
    assert all(list(x) == ["id", "source", "score", "lexicalScore", "fusedScore", "preview"] for x in rows)
    assert [(x["id"], x["score"], x["lexicalScore"], x["fusedScore"]) for x in rows] == [
        (h.id, h.score, h.lexical_score, h.fused_score) for h in want]
    assert rows[0]["id"] == "c17" and rows[0]["lexicalScore"] > 0
    lex = c.post("/rag/search", json={**body, "mode": "lexical"}).json()
    assert lex[0]["id"] == "c17" and all(x["lexicalScore"] > 0 and x["fusedScore"] > 0 for x in lex)
    for bad in ("x", "", 3, ["hybrid"]):
        r = c.post("/rag/search", json={**body, "mode": bad})
        assert r.status_code == 400 and "mode" in r.json()["error"], r.text
    # the configured default
    cfg = Config()
    cfg.rag.search_mode = "hybrid"
    idx._lex = None
    c2 = TestClient(create_rag_app(cfg, idx, build_index=False))
    assert idx._lex is not None  # built at start-up
    assert c2.post("/rag/search", json=body).json() == rows
    assert c2.post("/rag/search", json={**body, "mode": "dense"}).text == plain.text
    cfg.rag.search_mode = "fuzzy"
    with pytest.raises(ValueError, match="search_mode"):
        create_rag_app(cfg, idx, build_index=False)
    # a sharded corpus answers a non-dense mode with a 400 that says so
    idx.set_sharded(lambda qv, k: (torch.zeros(len(qv), k), torch.zeros(len(qv), k, dtype=torch.int32)), dim=128)
    r = c.post("/rag/search", json={**body, "mode": "hybrid"})
    assert r.status_code == 400 and "sharded" in r.json()["error"]


def test_config_defaults_and_overrides():
    from llm_kubernetes_minikube_sharp4dev_amd.config import load_config

    r = RagConfig()
    assert (r.search_mode, r.hybrid_candidates, r.rrf_k, r.bm25_k1, r.bm25_b) == ("dense", 24, 60, 1.2, 0.75)
    c = load_config(env={"LK_RAG__SEARCH_MODE": "hybrid", "LK_RAG__BM25_B": "0.5", "LK_RAG__RRF_K": "30"},
                    cli={"rag.hybrid_candidates": "32"})
    assert (c.rag.search_mode, c.rag.bm25_b, c.rag.rrf_k, c.rag.hybrid_candidates) == ("hybrid", 0.5, 30, 32)


def test_lexical_span_and_configured_parameters():
    from llm_kubernetes_minikube_sharp4dev_amd.utils import tracing

    idx = _index()
    idx.configure_lexical(hybrid_candidates=8, rrf_k=10, bm25_k1=2.0, bm25_b=0.0)
    hyb = idx.query(IDENT, 3, mode="hybrid")
    spans = [r for r in tracing.recent(20) if r["span"] == "rag.lexical"]
    assert spans and spans[-1]["component"] == "rag_index" and spans[-1]["mode"] == "hybrid" and spans[-1]["candidates"] == 8
    assert idx.lexical().k1 == 2.0 and torch.all(idx.lexical().kn == 2.0)      # b = 0: kn = k1
    hit = next(h for h in hyb if h.id == "c17")
    assert hit.fused_score >= 1 / 11                                           # rrf_k = 10, lexical rank 1
