"""Shared inputs of the BM25 tests (the fp32 reference on the CPU, csrc/bm25.hip on the GPU).

Exact probes.  kn == 1 for every document (k1 = 1, b = 0) and tf in {1, 3, 7, 15}, so
tf / (tf + kn) is one of 1/2, 3/4, 7/8, 15/16; the weights are in {1, 2, 4, 8}.  Every product is a
multiple of 1/16 and at most 8, so any sum of at most 64 of them is exact in fp32 in any order, and
a correctly rounded division is exact too.  Expected scores come from numpy int64 arithmetic in
sixteenths, ordered by (-score, id), and are compared bit for bit, ids included.  A second batch
has tf = 255 everywhere (impact 255/256, sums in 256ths, still exact).

The index is periodic in the document id with period 64 (which divides the kernel's chunk), so
equal scores occur inside a chunk and across chunks and the lower id has to win.  Terms:
  0      df = N (every document)
  1      df = 1, at document 0
  2      df = 1, at document N - 1
  3      an empty posting list
  4..69  documents d with d % 64 in a random set S_t
Queries, cycled by row: 64 terms; no term (all pads); the three rare / empty terms (fewer hits than
K: pads); term 0 alone (everything ties in groups); the empty term alone; a mix; then random ones.

Random postings: fp64 evaluation of the same f32 inputs and the kernel's error bound.
"""
import functools

import numpy as np
import torch

V_PROBE = 70
TFS = np.array([1, 3, 7, 15])
WS = np.array([1, 2, 4, 8])
IMP16 = np.zeros(16, dtype=np.int64)  # 16 * tf / (tf + 1)
IMP16[TFS] = [8, 12, 14, 15]


def _csr(lists, V):
    """[(term, docs ascending, tfs)] -> term_ptr int64, post_doc int32, post_tf uint8"""
    ptr = np.zeros(V + 1, dtype=np.int64)
    docs, tfs = [], []
    for t in range(V):
        d, f = lists[t]
        assert np.all(np.diff(d) > 0)
        ptr[t + 1] = ptr[t] + len(d)
        docs.append(np.asarray(d, dtype=np.int64))
        tfs.append(np.asarray(f, dtype=np.int64))
    doc = np.concatenate(docs) if docs else np.zeros(0, np.int64)
    tf = np.concatenate(tfs) if tfs else np.zeros(0, np.int64)
    return (torch.from_numpy(ptr), torch.from_numpy(doc.astype(np.int32)), torch.from_numpy(tf.astype(np.uint8)))


def _queries(nq, rng):
    """[(terms ascending, weights)] by row pattern"""
    w = lambda n: rng.choice(WS, size=n)  # noqa: E731
    out = []
    for i in range(nq):
        p = i % 7 if nq > 1 else 5
        if p == 0:
            t = np.arange(4, 68)
        elif p == 1:
            t = np.zeros(0, dtype=np.int64)
        elif p == 2:
            t = np.array([1, 2, 3])
        elif p == 3:
            t = np.array([0])
        elif p == 4:
            t = np.array([3])
        elif p == 5:
            t = np.concatenate([[0, 1, 2, 3], np.sort(rng.choice(np.arange(4, V_PROBE), size=10, replace=False))])
        else:
            t = np.sort(rng.choice(np.arange(V_PROBE), size=int(rng.integers(1, 20)), replace=False))
        out.append((t.astype(np.int64), w(len(t)).astype(np.int64)))
    return out


@functools.lru_cache(maxsize=None)
def exact_probe(N, nq, K, tf255=False, seed=0):
    """-> dict(term_ptr, post_doc, post_tf, kn, q_ptr, q_term, q_w, exp_s f32 [nq, K], exp_i int32 [nq, K])."""
    rng = np.random.default_rng(seed * 7919 + N * 31 + nq)
    d_all = np.arange(N, dtype=np.int64)
    units = 256 if tf255 else 16
    imp = np.zeros((V_PROBE, N), dtype=np.int64)  # impact of (term, doc) in 1/units, 0: no posting
    lists = []
    for t in range(V_PROBE):
        if t == 0:
            d = d_all
        elif t == 1:
            d = d_all[:1]
        elif t == 2:
            d = d_all[-1:]
        elif t == 3:
            d = d_all[:0]
        else:
            S = rng.choice(64, size=int(rng.integers(1, 33)), replace=False)
            d = d_all[np.isin(d_all % 64, S)]
        f = np.full(len(d), 255) if tf255 else TFS[((d % 64) * 5 + t) % 4]
        imp[t, d] = 255 if tf255 else IMP16[f]
        lists.append((d, f))
    term_ptr, post_doc, post_tf = _csr(lists, V_PROBE)
    qs = _queries(nq, rng)
    q_ptr = np.zeros(nq + 1, dtype=np.int32)
    exp_s = np.full((nq, K), -np.inf, dtype=np.float32)
    exp_i = np.full((nq, K), -1, dtype=np.int32)
    for i, (t, w) in enumerate(qs):
        q_ptr[i + 1] = q_ptr[i] + len(t)
        sc = (w[:, None] * imp[t]).sum(0) if len(t) else np.zeros(N, dtype=np.int64)
        assert sc.max(initial=0) < 2 ** 24
        hit = np.flatnonzero(sc > 0)
        order = hit[np.lexsort((hit, -sc[hit]))][:K]
        exp_s[i, :len(order)] = (sc[order].astype(np.float64) / units).astype(np.float32)
        exp_i[i, :len(order)] = order
    q_term = np.concatenate([t for t, _ in qs]).astype(np.int32)
    q_w = np.concatenate([w for _, w in qs]).astype(np.float32)
    return dict(term_ptr=term_ptr, post_doc=post_doc, post_tf=post_tf, kn=torch.ones(N, dtype=torch.float32),
                q_ptr=torch.from_numpy(q_ptr), q_term=torch.from_numpy(q_term), q_w=torch.from_numpy(q_w),
                exp_s=exp_s, exp_i=exp_i)


ARGS = ("term_ptr", "post_doc", "post_tf", "kn", "q_ptr", "q_term", "q_w")


def probe_args(p, device=None):
    """The op's positional tensor arguments, on ``device``."""
    return tuple(p[k] if device is None else p[k].to(device) for k in ARGS)


def check_exact(got_s, got_i, p, what=""):
    gs, gi = got_s.cpu().numpy(), got_i.cpu().numpy()
    assert gs.dtype == np.float32 and gi.dtype == np.int32 and gs.shape == p["exp_s"].shape == gi.shape
    assert np.array_equal(gi, p["exp_i"]), (what, np.argwhere(gi != p["exp_i"])[:5])
    assert np.array_equal(gs.view(np.uint32), p["exp_s"].view(np.uint32)), (what, np.argwhere(gs != p["exp_s"])[:5])


# ---- random postings: real kn, real idf weights, Zipf df
@functools.lru_cache(maxsize=None)
def random_index(N, V=500, nq=33, seed=0, k1=1.2, b=0.75):
    rng = np.random.default_rng(seed)
    dl = rng.integers(20, 400, size=N).astype(np.float64)
    kn = (k1 * (1.0 - b + b * dl / dl.mean())).astype(np.float32)
    lists = []
    df = np.zeros(V, dtype=np.int64)
    for t in range(V):
        df[t] = min(N, max(1, int(0.6 * N / (t + 1))))
        d = np.sort(rng.choice(N, size=df[t], replace=False))
        f = np.minimum(rng.geometric(0.45, size=df[t]), 255)
        lists.append((d, f))
    term_ptr, post_doc, post_tf = _csr(lists, V)
    idf = np.log(1.0 + (N - df + 0.5) / (df + 0.5))
    q_ptr, terms, ws = [0], [], []
    for i in range(nq):
        n = 64 if i == 0 else int(rng.integers(1, 13))
        # half of the draws from the frequent head, half from anywhere
        head = rng.choice(min(V, 40), size=min(n // 2, 40), replace=False)
        t = np.unique(np.concatenate([head, rng.choice(V, size=n - len(head), replace=False)]))[:64]
        qtf = rng.integers(1, 3, size=len(t))
        terms.append(t)
        ws.append((qtf * idf[t]).astype(np.float32))
        q_ptr.append(q_ptr[-1] + len(t))
    return dict(term_ptr=term_ptr, post_doc=post_doc, post_tf=post_tf, kn=torch.from_numpy(kn),
                q_ptr=torch.tensor(q_ptr, dtype=torch.int32),
                q_term=torch.from_numpy(np.concatenate(terms).astype(np.int32)),
                q_w=torch.from_numpy(np.concatenate(ws).astype(np.float32)))


def scores_fp64(p):
    """-> (score fp64 [nq, N], bound [nq, N]) of the f32 inputs: every impact is positive, so with T
    matched terms the fp32 result is within (T + 2) 2^-24 of the exact sum, relative -- tf + kn, the
    quotient and the product put three roundings on each impact, and each of the T - 1 adds one on a
    partial sum that is no larger than the whole."""
    tp = p["term_ptr"].numpy()
    pd = p["post_doc"].numpy().astype(np.int64)
    tf = p["post_tf"].numpy().astype(np.float64)
    kn = p["kn"].numpy().astype(np.float64)
    qp, qt, qw = p["q_ptr"].numpy(), p["q_term"].numpy(), p["q_w"].numpy().astype(np.float64)
    nq, N = len(qp) - 1, len(kn)
    sc = np.zeros((nq, N))
    T = np.zeros((nq, N))
    for q in range(nq):
        for j in range(qp[q], qp[q + 1]):
            t = qt[j]
            d = pd[tp[t]:tp[t + 1]]
            f = tf[tp[t]:tp[t + 1]]
            sc[q, d] += qw[j] * f / (f + kn[d])
            T[q, d] += 1
    return sc, (T + 2) * 2.0 ** -24 * sc


def check_within_bound(got_s, got_i, p, K):
    """Every returned score within the bound of its fp64 value; every returned id's fp64 score no
    lower than the fp64 K-th best minus the bound.  -> (max error, its bound, max error / bound)."""
    sc, bound = scores_fp64(p)
    gs, gi = got_s.double().cpu().numpy(), got_i.cpu().numpy()
    worst = (0.0, 0.0, 0.0)
    for q in range(sc.shape[0]):
        pos = np.sort(sc[q][sc[q] > 0])[::-1]
        n = min(K, len(pos))
        ids = gi[q, :n]
        assert np.all(ids >= 0) and np.all(gi[q, n:] == -1) and len(set(ids.tolist())) == n, (q, gi[q])
        err = np.abs(gs[q, :n] - sc[q, ids])
        assert np.all(err <= bound[q, ids]), (q, err.max(), bound[q, ids])
        if n:
            assert np.all(sc[q, ids] >= pos[n - 1] - bound[q, ids]), (q, ids)
            assert np.all(np.diff(gs[q, :n]) <= 0)
            j = int(np.argmax(err / bound[q, ids]))
            if err[j] / bound[q, ids][j] >= worst[2]:
                worst = (float(err[j]), float(bound[q, ids][j]), float(err[j] / bound[q, ids][j]))
    return worst


def _runbook(i, ident=None):
    from llm_kubernetes_minikube_sharp4dev_amd.rag.synthetic import make_document

    text = make_document(i, seed=5, target_chars=500)
    return text + (f"\nIl pod resta in {ident} finche' l'immagine non e' presente sul nodo." if ident else "")


def small_corpus(n=300, ident_at=137, ident="ErrImageNeverPull"):
    """A few hundred synthetic runbook chunks, exactly one of which contains ``ident``."""
    return [_runbook(i, ident if i == ident_at else None) for i in range(n)]
