"""csrc/mmr.hip on the GPU: the exact probes bit for bit (twice: the same bits on every run), random rows
with planted near-copies against fp64 within the derived bound, the refusals, the device chain kNN ->
MMR of RagIndex.search_vectors_async, and RagIndex.query end to end on both backends.
The probes, the model and the bound are in tests/mmr_probes.py; the derivation is in docs/mmr.md.

Measured on an MI355X (`pytest -s` prints it; D = 384 / 768, lam = 0.3 / 0.7): the worst |max_sim - fp64|
is 6.64e-03 of e_sim, every one of the 1,320 rounds picked the fp64 best (shortfall 0 of 2 e_mmr), and
the 318 to 329 of 330 rounds per case that fp64 decides beyond 2 e_mmr equal the fp32 reference's ids
(docs/mmr.md, "The bound")."""
import numpy as np
import pytest
import torch

import mmr_probes as P
from llm_kubernetes_minikube_sharp4dev_amd import ops
from llm_kubernetes_minikube_sharp4dev_amd.rag.embedder import HashEmbedder
from llm_kubernetes_minikube_sharp4dev_amd.rag.index import RagIndex

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_limit_exported(hip):
    assert int(hip.MMR_MAX_CAND) == ops.reference.MMR_MAX_CAND == 64


# ------------------------------------------------------------------ 1. exact probes
@pytest.mark.parametrize("D", P.SWEEP_D)
def test_exact_probes_bit_equal(hip, D):
    for d, C, K, nq, lam4 in P.sweep():
        if d != D:
            continue
        case = P.make_case(D, C, K, nq, lam4)
        corpus, cn, cid, rel, lam = P.tensors(case, DEV)
        out = hip.mmr_select(corpus, cn, cid, rel, lam, K)
        P.check_exact(out, case, (D, C, K, nq, lam4))
        # no atomics, one order for every sum: the same bits again, and through the ops entry point
        again = ops.mmr_select(corpus, cn, cid, rel, lam, K)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, again))


@pytest.mark.parametrize("lam4", P.LAMS4)
def test_every_lambda_on_the_full_width(hip, lam4):
    for D in (48, 768):
        case = P.make_case(D, 64, 64, 3, lam4)
        corpus, cn, cid, rel, lam = P.tensors(case, DEV)
        P.check_exact(hip.mmr_select(corpus, cn, cid, rel, lam, 64), case, (D, lam4))


# ------------------------------------------------------------------ 2. random rows vs fp64
@pytest.mark.parametrize("lam", [0.3, 0.7])
@pytest.mark.parametrize("D", [384, 768])
def test_random_rows_within_derived_bound(hip, D, lam):
    C, K = 64, 10
    X, Q = P.random_case(D)
    corpus, qs = X.to(DEV), Q.to(DEV)
    cn, qn = ops.row_norms(corpus), ops.row_norms(qs)
    rel, cid = ops.knn_topk(corpus, cn, qs, qn, C)
    out = hip.mmr_select(corpus, cn, cid, rel, lam, K)
    again = hip.mmr_select(corpus, cn, cid, rel, lam, K)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, again))
    ref = ops.reference.mmr_select(X, cn.cpu(), cid.cpu(), rel.cpu(), lam, K)
    w_sim, w_pick, compared = P.check_against_fp64(out, corpus, cn, cid, rel, lam, K, ref_ids=ref[1])
    near = int((out[4][:, 1:] > 0.9).sum())
    print(f"mmr_select D={D} lam={lam} N=1000 C={C} K={K} nq=33: worst |max_sim - fp64| / e_sim = {w_sim:.2e}, worst "
          f"(fp64 best - fp64 of the pick) / (2 e_mmr) = {w_pick:.2e}; {compared} of {33 * K} rounds decided beyond "
          f"2 e_mmr and equal to the fp32 reference; {near} picks had a near-copy (sim > 0.9) among the earlier ones")
    assert 0 < w_sim <= 1 and 0 <= w_pick <= 1 and compared > 33 * K // 2
    # the first pick is the top cosine
    assert torch.equal(out[1][:, 0], cid[:, 0]) and torch.all(out[4][:, 0] == 0)


# ------------------------------------------------------------------ 3. refusals
def test_refusals_raise_before_any_launch(hip):
    case = P.make_case(48, 33, 6, 3, 1)
    corpus, cn, cid, rel, lam = P.tensors(case, DEV)
    bad = [
        (r"C \(the width of cand_id\) must be in \[1, 64\]", (corpus, cn, cid.repeat(1, 2), rel.repeat(1, 2), lam, 6)),
        (r"C \(the width of cand_id\)", (corpus, cn, cid[:, :0].contiguous(), rel[:, :0].contiguous(), lam, 1)),
        (r"K must be", (corpus, cn, cid, rel, lam, 0)),
        (r"K must be", (corpus, cn, cid, rel, lam, 34)),
        (r"D must be a multiple of 16", (corpus[:, :40].contiguous(), cn, cid, rel, lam, 6)),
        (r"D must be a multiple of 16", (corpus.repeat(1, 22), cn, cid, rel, lam, 6)),
        (r"lam must be a finite number in \[0, 1\]", (corpus, cn, cid, rel, 1.5, 6)),
        (r"lam must be", (corpus, cn, cid, rel, -0.25, 6)),
        (r"lam must be", (corpus, cn, cid, rel, float("nan"), 6)),
        (r"lam must be", (corpus, cn, cid, rel, float("inf"), 6)),
        (r"same shape", (corpus, cn, cid, rel[:, :-1].contiguous(), lam, 6)),
        (r"bfloat16", (corpus.float(), cn, cid, rel, lam, 6)),
        (r"cnorm must be", (corpus, cn[:-1].contiguous(), cid, rel, lam, 6)),
        (r"int32", (corpus, cn, cid.long(), rel, lam, 6)),
        (r"float32", (corpus, cn, cid, rel.double(), lam, 6)),
        (r"GPU tensor", (corpus, cn, cid.cpu(), rel, lam, 6)),
    ]
    for match, args in bad:
        with pytest.raises(RuntimeError, match=match):
            hip.mmr_select(*args)
    for match, args in bad[:-1]:
        with pytest.raises(ValueError, match=match):
            ops.mmr_select(*args)
    # nothing was launched and the device is fine: the next call gives the probe's result
    P.check_exact(hip.mmr_select(corpus, cn, cid, rel, lam, 6), case)
    # no queries; no corpus rows (every candidate absent, no row is read)
    out = hip.mmr_select(corpus, cn, cid[:0].contiguous(), rel[:0].contiguous(), lam, 6)
    assert [tuple(o.shape) for o in out] == [(0, 6)] * 5
    out = hip.mmr_select(corpus[:0].contiguous(), cn[:0].contiguous(), cid, rel, lam, 6)
    assert torch.all(out[0] == -1) and torch.all(out[1] == -1) and all(torch.all(torch.isinf(o)) for o in out[2:])


# ------------------------------------------------------------------ 4. the device chain kNN -> MMR
@pytest.fixture(scope="module")
def probe_index():
    X = P.corpus(128)
    idx = RagIndex(HashEmbedder(128), backend="gpu", device=DEV)
    idx.add([f"c{i}" for i in range(P.N)], ["probe.md"] * P.N, [f"row {i}" for i in range(P.N)], X.astype(np.float32))
    return idx, X


@pytest.mark.parametrize("k", [1, 6])
@pytest.mark.parametrize("nq", [1, 33])
def test_search_vectors_async_chain(probe_index, nq, k):
    idx, X = probe_index
    Q = P.probe_queries(X, nq).astype(np.float32)
    corpus, norms = idx.gpu_tensors()
    assert torch.all(norms == 4)
    before = idx.search_vectors(Q, k)
    qt = torch.from_numpy(Q).to(DEV, torch.bfloat16)
    s, i = ops.knn_topk(corpus, norms, qt, ops.row_norms(qt), k)
    assert before == [list(zip(ir, sr)) for sr, ir in zip(s.tolist(), i.tolist())]
    assert idx.search_vectors_async(Q, k, mmr=None).result() == before
    assert idx.search_vectors_async(Q, k).result() == before
    for lam4, C in ((2, 24), (1, 64), (4, 24), (0, 3)):
        pool = min(64, max(k, C))
        cands = idx.search_vectors(Q, pool)
        ids = np.array([[d for d, _ in row] for row in cands])
        rel = np.array([[c for _, c in row] for row in cands])
        r16 = np.rint(rel * 16).astype(np.int64)
        assert ids.shape == (nq, pool) and np.array_equal(r16 / 16.0, rel)
        _, e_id, e_rel, _, _ = P.model(X, ids, r16, np.zeros(ids.shape, bool), lam4, k)
        want = [list(zip(ir, sr)) for sr, ir in zip(e_rel.tolist(), e_id.tolist())]
        got = idx.search_vectors_async(Q, k, mmr=(lam4 / 4.0, C)).result()
        assert got == want, (lam4, C)
        assert idx.search_vectors(Q, k, mmr=(lam4 / 4.0, C)) == want
        assert [row[0] for row in got] == [row[0] for row in before]        # the first pick: the top cosine
        if lam4 == 4:
            assert got == before                                           # lam = 1: the cosine order


# ------------------------------------------------------------------ 5. end to end
COPY_AT = (7, 3, 12, 9, 15)     # five exact copies; the lowest index is 3
DIST_AT = (20, 5, 11, 17)       # four distinct rows, in falling cosine order


def constructed_vectors():
    """D = 128, small integers (exact in bf16 and fp32).  The query direction is e0; the copies are
    4 e0 + 2 e1 (cosine 0.894), distinct row j is 4 e0 + (3 + j) e_{2+j} (cosines 0.8, 0.707, 0.625,
    0.555) and the filler e0 + 8 e_{6+i} (0.124).  With lam = 1/2, after the first copy every other copy
    has mmr 0.447 - 0.5 = -0.053, the distinct rows 0.042, 0.037, 0.033, 0.029 (their largest similarity
    is the one to the copy, 0.894 times their cosine, before and after each other's selection) and the
    filler 0.007: the copy, then the distinct rows in their cosine order."""
    n = 26
    V = np.zeros((n, 128), np.float32)
    fill = 0
    for i in range(n):
        V[i, 0] = 4
        if i in COPY_AT:
            V[i, 1] = 2
        elif i in DIST_AT:
            j = DIST_AT.index(i)
            V[i, 2 + j] = 3 + j
        else:
            V[i, 0] = 1
            V[i, 6 + fill] = 8
            fill += 1
    q = np.zeros(128, np.float32)
    q[0] = 1
    return V, q


class FixedEmbedder:
    model = "fixed"

    def __init__(self, q):
        self.q = q

    def embed(self, texts):
        return np.stack([self.q for _ in texts])


def test_query_end_to_end_on_both_backends():
    V, q = constructed_vectors()
    res = {}
    for backend, dev in (("gpu", DEV), ("exact", "cpu")):
        idx = RagIndex(FixedEmbedder(q), backend=backend, device=dev)
        idx.add([f"c{i}" for i in range(len(V))], ["m.md"] * len(V), [f"text {i}" for i in range(len(V))], V)
        plain = idx.query("anything", top_k=5)
        assert [h.id for h in plain] == [f"c{i}" for i in sorted(COPY_AT)]
        assert all(h.mmr_score is None and h.max_sim is None for h in plain)
        hits = idx.query("anything", top_k=5, mmr_lambda=0.5)
        assert [h.id for h in hits] == ["c3"] + [f"c{i}" for i in DIST_AT]
        cos = [4 / np.sqrt(20)] + [4 / np.sqrt(16 + (3 + j) ** 2) for j in range(4)]
        assert [h.score for h in hits] == pytest.approx(cos, abs=1e-6)                  # still the cosine
        assert hits[0].max_sim == 0 and hits[0].mmr_score == pytest.approx(0.5 * cos[0], abs=1e-6)
        # no copy but the first is in the result; what the others report is their similarity to it
        assert [h.max_sim for h in hits[1:]] == pytest.approx([cos[0] * c for c in cos[1:]], abs=1e-6)
        assert [h.mmr_score for h in hits[1:]] == pytest.approx([0.5 * c - 0.5 * cos[0] * c for c in cos[1:]], abs=1e-6)
        res[backend] = [h.id for h in hits]
    assert res["gpu"] == res["exact"]
