"""csrc/bm25.hip on the GPU: the exact probes bit for bit (twice: the same bits on every run), random
postings against an fp64 evaluation of the same f32 inputs within the derived bound, the refusals,
and RagIndex lexical / hybrid search on the GPU against the same index on the CPU reference path.
The probes and the bound are in tests/bm25_probes.py.

Measured on an MI355X (random postings, N = 3C+5, V = 500, nq = 33, K = 10; `pytest -s` prints it):
the worst returned score is 9.142e-07 from its fp64 value against a bound of 1.520e-06 (ratio
0.601), and the output equals the fp32 reference's bit for bit (docs/hybrid_search.md)."""
import numpy as np
import pytest
import torch

import bm25_probes as P
from llm_kubernetes_minikube_sharp4dev_amd import ops
from llm_kubernetes_minikube_sharp4dev_amd.rag.embedder import HashEmbedder
from llm_kubernetes_minikube_sharp4dev_amd.rag.index import RagIndex

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = ops.reference.BM25_CHUNK


def test_chunk_size_exported(hip):
    assert int(hip.BM25_CHUNK) == C and int(hip.BM25_MAX_TERMS) == ops.reference.BM25_MAX_TERMS == 64


# ------------------------------------------------------------------ 1. exact probes
@pytest.mark.parametrize("tf255", [False, True])
@pytest.mark.parametrize("N", [1, C - 1, C, C + 1, 3 * C + 5])
def test_exact_probes_bit_equal(hip, N, tf255):
    for nq in (1, 3, 33):
        for K in (1, 5, 64):
            p = P.exact_probe(N, nq, K, tf255)
            a = P.probe_args(p, DEV)
            s, i = hip.bm25_topk(*a, K)
            P.check_exact(s, i, p, (N, nq, K, tf255))
            # no atomics, one summation order: the same bits again; and through the ops entry
            # point with q_ptr left on the host
            s2, i2 = ops.bm25_topk(*a[:4], p["q_ptr"], a[5], a[6], K)
            assert torch.equal(s2, s) and torch.equal(i2, i)


# ------------------------------------------------------------------ 2. random postings vs fp64
def test_random_postings_within_derived_bound(hip):
    K = 10
    r = P.random_index(3 * C + 5)
    a = P.probe_args(r, DEV)
    s, i = hip.bm25_topk(*a, K)
    err, bound, ratio = P.check_within_bound(s, i, r, K)
    print(f"bm25_topk N={3 * C + 5} V=500 nq=33 K={K}: worst |score - fp64| {err:.3e} against its bound {bound:.3e} "
          f"(ratio {ratio:.3f})")
    assert 0 < ratio <= 1
    s2, i2 = hip.bm25_topk(*a, K)
    assert torch.equal(s2, s) and torch.equal(i2, i)
    # the kernel rounds the quotient, the product and the add once each, in the reference's order
    rs, ri = ops.reference.bm25_topk(*P.probe_args(r), K)
    same = bool(torch.equal(rs, s.cpu()) and torch.equal(ri, i.cpu()))
    print(f"bm25_topk equals the fp32 reference bit for bit: {same}")
    assert same


# ------------------------------------------------------------------ 3. refusals
def test_refusals_raise_before_any_launch(hip):
    p = P.exact_probe(C + 1, 3, 5)
    a = P.probe_args(p, DEV)
    with pytest.raises(RuntimeError, match=r"bm25_topk: unsupported shape/config \(code -1\)"):
        hip.bm25_topk(*a, 65)
    with pytest.raises(RuntimeError, match=r"unsupported shape/config \(code -1\)"):
        hip.bm25_topk(*a, 0)
    qp = torch.tensor([0, 65], dtype=torch.int32, device=DEV)
    qt = torch.arange(65, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match=r"unsupported shape/config \(code -2\)"):
        hip.bm25_topk(*a[:4], qp, qt, torch.ones(65, device=DEV), 5)
    with pytest.raises(RuntimeError, match="q_ptr must run from 0"):
        hip.bm25_topk(*a[:4], a[4][:-1].contiguous(), a[5], a[6], 5)      # ends short of the terms
    bad = a[4].clone()
    bad[1] = bad[2] + 1
    with pytest.raises(RuntimeError, match="non-decreasing"):
        hip.bm25_topk(*a[:4], bad, a[5], a[6], 5)
    with pytest.raises(RuntimeError, match="q_term / q_w"):
        hip.bm25_topk(*a[:4], a[4], a[5], a[6][:-1].contiguous(), 5)
    # nothing was launched and the device is fine: the next call gives the probe's result
    s, i = hip.bm25_topk(*a, 5)
    P.check_exact(s, i, p)
    # no queries, no documents
    e = torch.zeros(0, dtype=torch.int32, device=DEV)
    s, i = hip.bm25_topk(*a[:4], torch.zeros(1, dtype=torch.int32, device=DEV), e, e.float(), 5)
    assert s.shape == (0, 5) and i.shape == (0, 5)


# ------------------------------------------------------------------ 4. end to end
IDENT = "ErrImageNeverPull"


@pytest.fixture(scope="module")
def indexes():
    texts = P.small_corpus(300, 137, IDENT)
    emb = HashEmbedder(128)
    vec = emb.embed(texts)
    out = []
    for backend, dev in (("gpu", DEV), ("exact", "cpu")):
        idx = RagIndex(emb, backend=backend, device=dev)
        idx.add([f"c{i}" for i in range(len(texts))], ["runbook.md"] * len(texts), texts, vec)
        out.append(idx)
    return out


def test_rag_index_lexical_matches_the_cpu_path(indexes):
    g, c = indexes
    assert g.lexical().post_doc.is_cuda and not c.lexical().post_doc.is_cuda
    for k in ("term_ptr", "post_doc", "post_tf", "kn"):
        assert torch.equal(getattr(g.lexical(), k).cpu(), getattr(c.lexical(), k))
    lex = c.lexical()
    queries = ["scalare il deployment nel namespace staging", "log del pod in errore", "rollout rollback release",
               IDENT, "readiness probe soglia latenza memoria", "zzzz"]
    K = 24
    enc = lex.encode(queries)
    p = dict(term_ptr=lex.term_ptr, post_doc=lex.post_doc, post_tf=lex.post_tf, kn=lex.kn, q_ptr=enc[0],
             q_term=enc[1], q_w=enc[2])
    sc, bound = P.scores_fp64(p)
    got = g.lexical().search(queries, K)
    want = c.lexical().search(queries, K)
    assert got[-1] == [] and want[-1] == []
    for q in range(len(queries)):
        gi, wi = [d for d, _ in got[q]], [d for d, _ in want[q]]
        assert len(gi) == len(wi)
        for r, (a, b) in enumerate(zip(gi, wi)):
            # the ids agree wherever the fp64 scores of adjacent ranks differ by more than the bound
            if a != b:
                assert abs(sc[q, a] - sc[q, b]) <= bound[q, a] + bound[q, b], (q, r, a, b)
        for d, s in got[q]:
            assert abs(s - sc[q, d]) <= bound[q, d]


def test_rag_index_hybrid_on_the_gpu(indexes):
    g, c = indexes
    lex = g.query(IDENT, 5, mode="lexical")
    assert [h.id for h in lex] == ["c137"] and lex[0].fused_score == 1 / 61 and lex[0].lexical_score > 0
    hyb = g.query(IDENT, 5, mode="hybrid")
    assert len(hyb) == 5 and "c137" in [h.id for h in hyb[:2]]
    hit = next(h for h in hyb if h.id == "c137")
    assert hit.fused_score >= 1 / 61 and hit.lexical_score == lex[0].lexical_score
    # `score` stays the cosine of the bf16 scan, also for a hit that only the lexical list found
    scan = dict(g.search_vectors(g.embedder.embed([IDENT]), 64)[0])
    for h in hyb + lex:
        d = int(h.id[1:])
        want = scan[d] if d in scan else c.cosines(c.embedder.embed([IDENT])[0], [d])[0]
        assert h.score == pytest.approx(want, abs=2e-2 if d not in scan else 2e-6)
    g.configure_lexical(hybrid_candidates=2)
    try:
        q = "scalare il deployment " + IDENT
        few = g.query(q, 2, mode="hybrid")
        full = dict(g.search_vectors(g.embedder.embed([q]), 64)[0])
        assert all(h.score == pytest.approx(full[int(h.id[1:])], abs=2e-6) for h in few if int(h.id[1:]) in full)
    finally:
        g.configure_lexical()
