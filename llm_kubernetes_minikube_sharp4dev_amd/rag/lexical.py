"""Lexical (BM25) side of hybrid retrieval: the analyser, the inverted index and the query encoder.

Runbook queries are full of exact identifiers (``ImagePullBackOff``, ``OOMKilled``, a flag, a
deployment name) that dense embedders blur.  This module scores text lexically; the posting scan
itself is ``ops.bm25_topk`` (``csrc/bm25.hip`` on the GPU, an fp32 reference on the CPU) and
:meth:`RagIndex.query` fuses its list with the cosine list (docs/hybrid_search.md).

Analyser.  For every maximal run of Unicode letters and digits (``[^\\W_]+``) of at most 64
characters: the run, lower-cased; and, when the run splits into two or more parts at lower->Upper
boundaries, at letter<->digit boundaries and before the last capital of an all-caps prefix
(``HTTPServer`` -> ``HTTP``, ``Server``), each part of length >= 2, lower-cased.  So
``CrashLoopBackOff`` emits ``crashloopbackoff crash loop back off`` and the query "crash loop"
matches it.  No stemming, no stop list.  (The built-in BPE tokenizer is not an analyser: it cuts
``kubectl`` into ``k ub ect l`` and its word-initial pieces carry a leading space.)

Index.  Term ids follow the lexicographic order of the terms (independent of insertion order).
CSR by term: ``term_ptr`` int64 [V+1]; ``post_doc`` int32 [nnz], strictly ascending inside a term
(a document appears once per term -- the kernel relies on it, so it is asserted at build);
``post_tf`` uint8 [nnz], the term frequency clamped to 255; ``kn`` f32 [N] = k1 (1 - b + b dl_d /
avgdl) with dl_d the number of terms emitted for document d; df_t = term_ptr[t+1] - term_ptr[t].

Query.  Analysed like a document, unknown terms dropped, duplicates merged into qtf;
w_t = qtf ln(1 + (N - df + 0.5) / (df + 0.5)) in float64, stored as f32; at most 64 unique terms
(the 64 of highest w_t, ties to the lower id), sent ascending by id.
"""
from __future__ import annotations

import math
import re
import time
from collections import Counter
from typing import Optional, Sequence

import numpy as np
import torch

from .. import ops
from ..utils.logging import get_logger

log = get_logger("rag")

MAX_RUN = 64          # longer runs (hashes, base64) are dropped
MAX_QUERY_TERMS = 64  # csrc/kernels.h kLkBm25MaxTerms
_RUN = re.compile(r"[^\W_]+")
_CACHE: dict = {}
_CACHE_MAX = 1 << 18


def split_run(run: str) -> list[str]:
    """The parts of one letter/digit run (original case): cut at lower->Upper, at letter<->digit,
    and before the last capital of an all-caps prefix that a lower-case letter follows."""
    parts, start, n = [], 0, len(run)
    for i in range(1, n):
        a, c = run[i - 1], run[i]
        cut = (a.islower() and c.isupper()) or (a.isalpha() != c.isalpha()) or (
            a.isupper() and c.isupper() and i + 1 < n and run[i + 1].islower())
        if cut:
            parts.append(run[start:i])
            start = i
    parts.append(run[start:])
    return parts


def _run_terms(run: str) -> tuple:
    t = _CACHE.get(run)
    if t is None:
        if len(run) > MAX_RUN:
            t = ()
        else:
            parts = split_run(run)
            t = (run.lower(),) + (tuple(p.lower() for p in parts if len(p) >= 2) if len(parts) >= 2 else ())
        if len(_CACHE) < _CACHE_MAX:
            _CACHE[run] = t
    return t


def analyse(text: str) -> list[str]:
    """The terms of ``text``, in order of appearance (see the module docstring)."""
    out: list[str] = []
    for run in _RUN.findall(text):
        out.extend(_run_terms(run))
    return out


class LexicalIndex:
    """Inverted BM25 index over ``texts`` (document id = position), tensors on ``device``."""

    def __init__(self, texts: Sequence[str], k1: float = 1.2, b: float = 0.75, device="cpu"):
        t0 = time.perf_counter()
        self.k1, self.b = float(k1), float(b)
        self.device = torch.device(device)
        N = self.N = len(texts)
        prov: dict[str, int] = {}  # term -> provisional id (insertion order), remapped below
        p_term, p_doc, p_tf = [], [], []
        dl = np.zeros(N, dtype=np.int64)
        for d, text in enumerate(texts):
            terms = analyse(text)
            dl[d] = len(terms)
            for term, tf in Counter(terms).items():
                p_term.append(prov.setdefault(term, len(prov)))
                p_doc.append(d)
                p_tf.append(tf)
        self.terms = sorted(prov)
        self.term_id = {t: i for i, t in enumerate(self.terms)}
        V = self.V = len(self.terms)
        remap = np.zeros(max(V, 1), dtype=np.int64)
        for t, i in self.term_id.items():
            remap[prov[t]] = i
        term = remap[np.asarray(p_term, dtype=np.int64)] if p_term else np.zeros(0, dtype=np.int64)
        doc = np.asarray(p_doc, dtype=np.int64)
        tf = np.asarray(p_tf, dtype=np.int64)
        order = np.lexsort((doc, term))
        term, doc, tf = term[order], doc[order], tf[order]
        # the kernel adds each posting into its document's slot without atomics: one posting per
        # (term, document), ascending
        assert np.all((np.diff(term) > 0) | (np.diff(doc) > 0)), "postings must be strictly ascending inside a term"
        assert N < 2 ** 31
        term_ptr = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(np.bincount(term, minlength=V), out=term_ptr[1:])
        self.dl = dl
        self.avgdl = float(dl.mean()) if N and dl.sum() > 0 else 1.0
        kn = self.k1 * (1.0 - self.b + self.b * dl.astype(np.float64) / self.avgdl)
        self.df = np.diff(term_ptr)
        self.nnz = int(len(doc))
        self.term_ptr = torch.from_numpy(term_ptr).to(self.device)
        self.post_doc = torch.from_numpy(doc.astype(np.int32)).to(self.device)
        self.post_tf = torch.from_numpy(np.minimum(tf, 255).astype(np.uint8)).to(self.device)
        self.kn = torch.from_numpy(kn.astype(np.float32)).to(self.device)
        self.build_s = time.perf_counter() - t0
        log.info("[RAG] lexical index: N=%d V=%d nnz=%d built in %.3f s (%d bytes on %s)", N, V, self.nnz,
                 self.build_s, self.nbytes, self.device)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.term_ptr, self.post_doc, self.post_tf, self.kn))

    def idf(self, t: int) -> float:
        df = float(self.df[t])
        return math.log(1.0 + (self.N - df + 0.5) / (df + 0.5))

    def encode_one(self, query: str) -> tuple[list[int], list[float]]:
        """(term ids ascending, weights) of one query."""
        qtf = Counter(self.term_id[t] for t in analyse(query) if t in self.term_id)
        w = {t: n * self.idf(t) for t, n in qtf.items()}
        keep = sorted(w, key=lambda t: (-float(np.float32(w[t])), t))[:MAX_QUERY_TERMS]
        keep.sort()
        return keep, [w[t] for t in keep]

    def encode(self, queries: Sequence[str]):
        """-> (q_ptr int32 [nq+1], q_term int32 [nt], q_w f32 [nt]), on the host."""
        ptr, terms, ws = [0], [], []
        for q in queries:
            t, w = self.encode_one(q)
            terms += t
            ws += w
            ptr.append(len(terms))
        return (torch.tensor(ptr, dtype=torch.int32), torch.tensor(terms, dtype=torch.int32),
                torch.tensor(np.asarray(ws, dtype=np.float64).astype(np.float32)))

    def sum_df(self, query: str) -> int:
        """Postings a query scans: the work of the kernel."""
        return int(sum(self.df[t] for t in self.encode_one(query)[0]))

    def topk(self, q_ptr, q_term, q_w, K: int):
        """ops.bm25_topk over this index for encoded queries (q_ptr stays on the host: the op checks it there)."""
        return ops.bm25_topk(self.term_ptr, self.post_doc, self.post_tf, self.kn, q_ptr,
                             q_term.to(self.device), q_w.to(self.device), K)

    def search(self, queries: Sequence[str], K: int) -> list[list[tuple[int, float]]]:
        """Per query [(document, BM25 score)], score descending then id ascending, hits only."""
        K = max(1, min(int(K), 64))
        if self.N == 0 or not len(queries):
            return [[] for _ in queries]
        s, i = self.topk(*self.encode(queries), K)
        return [[(d, sc) for sc, d in zip(sr, ir) if d >= 0] for sr, ir in zip(s.tolist(), i.tolist())]


__all__ = ["analyse", "split_run", "LexicalIndex", "MAX_RUN", "MAX_QUERY_TERMS"]
