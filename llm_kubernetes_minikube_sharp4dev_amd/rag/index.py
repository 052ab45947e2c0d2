"""In-memory vector store — the MI355X counterpart of ``Helpers/RagIndex.cs``.

Ingestion (``RagIndex.cs:14-56``): recursive enumeration of ``.md/.txt/.yaml/.yml``
(case-insensitive), UTF-8 read, header split / sliding window, sanitize, skip blank
chunks, chunk id ``"{filename}#{i}"`` (``i`` counts kept chunks), source = path,
``[RAG]`` log lines; a missing folder logs a warning and leaves the index empty.
Unlike the reference (one HTTP embedding round-trip per chunk, serially) chunks
are embedded in large GPU batches.

Query (``RagIndex.cs:59-67``): embed the query, cosine against EVERY chunk, stable
descending sort, take ``max(1, topK)``.  Backends:

* ``exact`` — the reference's arithmetic: f32 products accumulated in f64,
  ``dot / (sqrt(na)*sqrt(nb) + 1e-9)``; dimension mismatch scores -1.
* ``gpu``   — corpus matrix resident in HBM (bf16 + f32 norms); the fused HIP
  cosine + top-k kernel (``csrc/knn.hip``) with the same tie order.

Checkpoint/resume: :meth:`save` / :meth:`load` persist embeddings +
metadata (safetensors + JSON) keyed by file content hash, so a restart re-embeds
only changed files.
"""
from __future__ import annotations

import hashlib
import json
import os
import threading
import time
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch

from .. import ops
from ..config import SEARCH_MODES, mmr_lambda_ok
from ..utils import metrics as M
from ..utils.logging import get_logger
from ..utils.tracing import Tracer
from .chunking import chunk_document, chunk_sliding, is_blank, sanitize, split_by_markdown_headers

log = get_logger("rag")

EXTENSIONS = (".md", ".txt", ".yaml", ".yml")
_tracer = Tracer("rag_index")


@dataclass
class RagChunk:                      # record RagChunk(Id, Source, Text, Embedding) — Program.cs:326
    id: str
    source: str
    text: str


@dataclass
class RagHit:                        # record RagHit(Id, Source, Text, double Score) — Program.cs:327
    id: str
    source: str
    text: str
    score: float
    rerank_score: Optional[float] = None  # set by RagIndex.query(..., reranker=...)
    lexical_score: Optional[float] = None  # BM25, modes 'lexical' / 'hybrid'; None: not in the lexical list
    fused_score: Optional[float] = None    # reciprocal-rank fusion score, modes 'lexical' / 'hybrid'
    mmr_score: Optional[float] = None      # MMR value at the time of the pick (query(..., mmr_lambda=...))
    max_sim: Optional[float] = None        # largest similarity to an earlier pick (0 for the first)


def cosine_exact(a: np.ndarray, b: np.ndarray) -> float:
    """``RagIndex.Cosine``: f32 element products, f64 accumulation, +1e-9."""
    if a.shape[-1] != b.shape[-1]:
        return -1.0
    a = a.astype(np.float32)
    b = b.astype(np.float32)
    dot = float(np.sum((a * b).astype(np.float64)))
    na = float(np.sum((a * a).astype(np.float64)))
    nb = float(np.sum((b * b).astype(np.float64)))
    return dot / (np.sqrt(na) * np.sqrt(nb) + 1e-9)


def rrf_fuse(lists: Sequence[Sequence[int]], rrf_k: int = 60) -> dict[int, float]:
    """Reciprocal-rank fusion of ranked id lists: fused(d) = sum over the lists holding d of
    1 / (rrf_k + rank), rank 1-based.  Order by (-fused, id)."""
    fused: dict[int, float] = {}
    for ranked in lists:
        for rank, d in enumerate(ranked, 1):
            fused[d] = fused.get(d, 0.0) + 1.0 / (rrf_k + rank)
    return fused


MMR_MAX_CANDIDATES = 64  # csrc/kernels.h kLkMmrMaxCand
_SHARDED_MMR = "MMR is not supported with a sharded (tensor-parallel) corpus: leave mmr_lambda unset"


def _check_mmr_lambda(lam) -> float:
    if not mmr_lambda_ok(lam):
        raise ValueError(f"mmr_lambda must be a number between 0 and 1 (got {lam!r})")
    return float(lam)


def mmr_select_f64(rows: np.ndarray, rel: Sequence[float], lam: float, K: int) -> list[tuple[int, float, float]]:
    """Greedy MMR (docs/mmr.md) over the candidates ``rows`` f32 [C, D] in float64, the exact backend's
    counterpart of ``ops.mmr_select``: similarities in the arithmetic of :func:`cosine_exact` (f32
    products, f64 sums), ``mmr_i = lam * rel_i - (1 - lam) * m_i`` with ``m_i`` 0 in the first round
    and afterwards the largest similarity to a pick (assigned from the first pick), ties to the lower
    position; a NaN ``rel`` is absent.  -> at most K picks [(position, mmr, max_sim)]."""
    rows = np.asarray(rows, dtype=np.float32)
    C = len(rows)
    nrm = np.sqrt((rows * rows).astype(np.float64).sum(1)) if C else np.zeros(0)
    relv = np.asarray(rel, dtype=np.float64)
    avail = ~np.isnan(relv)
    m = np.zeros(C)
    out: list[tuple[int, float, float]] = []
    for r in range(min(K, C)):
        v = lam * relv - (1.0 - lam) * m
        ok = avail & ~np.isnan(v)
        if not ok.any():
            break
        p = min((i for i in range(C) if ok[i]), key=lambda i: (-v[i], i))
        out.append((p, float(v[p]), float(m[p])))
        avail[p] = False
        sim = (rows * rows[p][None, :]).astype(np.float64).sum(1) / (nrm * nrm[p] + 1e-9)
        m = sim if r == 0 else np.maximum(m, sim)
    return out


def enumerate_files(folder: str) -> list[str]:
    out = []
    for root, _dirs, files in os.walk(folder):
        for f in files:
            if f.lower().endswith(EXTENSIONS):
                out.append(os.path.join(root, f))
    return sorted(out)


class RagIndex:
    def __init__(self, embedder, backend: str = "auto", device: Optional[str] = None,
                 gpu_threshold: int = 20000):
        self.embedder = embedder
        self.backend = backend
        self.device = torch.device(device) if device else (
            torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu"))
        self.gpu_threshold = gpu_threshold
        self.chunks: list[RagChunk] = []
        self._emb: list[np.ndarray] = []       # host f32 rows (exact backend / persistence)
        self._mat: Optional[np.ndarray] = None
        self._gpu = None                       # (corpus bf16, norms f32) on device
        self.file_hashes: dict[str, str] = {}
        # lexical side of hybrid search (rag/lexical.py): built lazily from the chunk texts, never
        # persisted; RagConfig's hybrid_candidates / rrf_k / bm25_k1 / bm25_b (configure_lexical)
        self._lex = None
        self._lex_lock = threading.Lock()
        self.hybrid_candidates, self.rrf_k, self.bm25_k1, self.bm25_b = 24, 60, 1.2, 0.75

    # ------------------------------------------------------------ ingestion
    def __len__(self):
        return len(self.chunks)

    def add(self, ids: Sequence[str], sources: Sequence[str], texts: Sequence[str], emb: np.ndarray):
        for i, s, t, e in zip(ids, sources, texts, emb):
            self.chunks.append(RagChunk(i, s, t))
            self._emb.append(np.asarray(e, dtype=np.float32))
        self._mat = None
        self._gpu = None
        self._lex = None

    def build_from_folder(self, folder: str, chunk_size: int = 800, overlap: int = 120,
                          batch_chunks: int = 4096) -> int:
        if not os.path.isdir(folder):
            log.warning("[RAG] Cartella non trovata: %s", folder)
            return 0
        files = enumerate_files(folder)
        log.info("[RAG] File trovati in %s: %d", folder, len(files))
        pend_ids, pend_src, pend_txt = [], [], []

        def flush():
            if pend_txt:
                self.add(pend_ids, pend_src, pend_txt, self.embedder.embed(pend_txt))
                pend_ids.clear(), pend_src.clear(), pend_txt.clear()

        for path in files:
            log.info("[RAG] Indicizzo file: %s", path)
            with open(path, "rb") as fh:
                raw = fh.read()
            self.file_hashes[path] = hashlib.sha256(raw).hexdigest()
            text = raw.decode("utf-8", errors="replace")
            if text.startswith("﻿"):
                text = text[1:]  # File.ReadAllTextAsync(UTF8) drops the BOM
            chunks = chunk_document(text, chunk_size, overlap)
            name = os.path.basename(path)
            for i, c in enumerate(chunks):
                pend_ids.append(f"{name}#{i}")
                pend_src.append(path)
                pend_txt.append(c)
            log.info("[RAG] Chunks dal file %s: %d", path, len(chunks))
            if len(pend_txt) >= batch_chunks:
                flush()
        flush()
        log.info("[RAG] Totale chunks indicizzati: %d", len(self.chunks))
        return len(self.chunks)

    # ------------------------------------------------------------ query
    def matrix(self) -> np.ndarray:
        if self._mat is None:
            self._mat = np.stack(self._emb) if self._emb else np.zeros((0, 0), np.float32)
        return self._mat

    def _use_gpu(self) -> bool:
        if self.backend == "gpu":
            local = True
        elif self.backend == "exact":
            local = False
        else:
            local = self.device.type == "cuda" and len(self.chunks) >= self.gpu_threshold
        if getattr(self, "_sharded", None) is not None:
            # the sharded scan ranks exactly like the single-GPU bf16 scan; where this process
            # would score on the host instead (backend 'exact', or 'auto' below the threshold) and
            # still holds the fp32 matrix, it does -- so a TP server ranks near-ties like TP=1
            return local or not self._emb
        return local

    def gpu_tensors(self):
        if self._gpu is None:
            corpus = torch.from_numpy(self.matrix()).to(self.device, torch.bfloat16).contiguous()
            self._gpu = (corpus, ops.row_norms(corpus))
        return self._gpu

    def set_gpu_corpus(self, corpus_bf16: torch.Tensor, norms: Optional[torch.Tensor] = None):
        """Attach a corpus matrix produced directly on the GPU (bulk index builds)."""
        self._gpu = (corpus_bf16.contiguous(), norms if norms is not None else ops.row_norms(corpus_bf16))

    def set_sharded(self, search_fn, dim: Optional[int] = None):
        """Route searches through a corpus-sharded kNN: ``search_fn(queries [nq, D] bf16, k) ->
        (scores f32 [nq, k], ids int32 [nq, k])`` (parallel.tp_engine.tp_knn_search: every TP
        rank scans its shard, merged in the single-scan order).  None restores the local scan.
        With a sharded search this process keeps no device copy of the corpus; ``dim`` (the
        corpus width) lets a mismatched query fail here rather than inside the sharded kNN."""
        self._sharded = search_fn
        self._sharded_dim = dim
        if search_fn is not None:
            self._gpu = None

    def search_vectors_async(self, q: np.ndarray | torch.Tensor, top_k: int,
                             mmr: Optional[tuple[float, int]] = None) -> "PendingSearch":
        """Launch a batched search without blocking the host: on the GPU the kNN kernel and
        one non-blocking copy of its (scores, ids) into pinned memory are enqueued on the
        current stream behind an event; :meth:`PendingSearch.result` waits for that event
        only (an engine thread collects it after its next step, when it has long completed).
        Elsewhere the search runs synchronously.

        ``mmr = (lam, C)``: the kNN returns ``min(64, max(top_k, C))`` hits and ``ops.mmr_select``
        (docs/mmr.md) picks ``top_k`` of them on the kNN's device outputs, on the same stream; the
        rows keep their type, [(chunk_index, cosine)], now in MMR order."""
        k = max(1, top_k)
        n = len(self.chunks)
        if mmr is not None:
            lam, pool = _check_mmr_lambda(mmr[0]), min(MMR_MAX_CANDIDATES, max(k, int(mmr[1])))
            if getattr(self, "_sharded", None) is not None:
                raise ValueError(_SHARDED_MMR)
        if n == 0 or not self._use_gpu():
            return PendingSearch(done=self.search_vectors(q, top_k, mmr) if n else [[] for _ in range(len(q))])
        qt = torch.as_tensor(q)
        sharded = getattr(self, "_sharded", None)
        if sharded is not None:
            # the shard's dtype (bf16 on the GPU, f32 on the CPU) is applied by the search
            dim = getattr(self, "_sharded_dim", None)
            if dim is not None and qt.shape[-1] != dim:
                raise ValueError(f"query width {qt.shape[-1]} != corpus width {dim}")
            s, i = sharded(qt.reshape(-1, qt.shape[-1]), min(k, 64))
        else:
            corpus, norms = self.gpu_tensors()
            # host queries are cast on the host (a few KB) and copied once: no device cast kernel
            qt = (qt.to(torch.bfloat16).to(self.device) if qt.device.type == "cpu"
                  else qt.to(self.device, torch.bfloat16)).reshape(-1, corpus.shape[1]).contiguous()
            qn = ops.row_norms(qt) if qt.is_cuda else qt.float().norm(dim=-1)
            if mmr is None:
                s, i = ops.knn_topk(corpus, norms, qt, qn, min(k, 64))
            else:
                cs, ci = ops.knn_topk(corpus, norms, qt, qn, pool)
                _, i, s, _, _ = ops.mmr_select(corpus, norms, ci, cs, lam, min(k, pool))
        if not s.is_cuda:
            return PendingSearch(done=_rows(s.tolist(), i.tolist(), min(k, n)))
        hs = torch.empty(s.shape, dtype=s.dtype, pin_memory=True)
        hi = torch.empty(i.shape, dtype=i.dtype, pin_memory=True)
        hs.copy_(s, non_blocking=True)
        hi.copy_(i, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return PendingSearch(host=(hs, hi, min(k, n)), event=ev)

    def search_vectors(self, q: np.ndarray | torch.Tensor, top_k: int,
                       mmr: Optional[tuple[float, int]] = None) -> list[list[tuple[int, float]]]:
        """Batched: q [nq, D] -> per query [(chunk_index, score)] (stable order); with ``mmr =
        (lam, C)`` the MMR selection of ``top_k`` among the best ``min(64, max(top_k, C))``."""
        k = max(1, top_k)
        n = len(self.chunks)
        if mmr is not None:
            lam, pool = _check_mmr_lambda(mmr[0]), min(MMR_MAX_CANDIDATES, max(k, int(mmr[1])))
            if getattr(self, "_sharded", None) is not None:
                raise ValueError(_SHARDED_MMR)
        if n == 0:
            return [[] for _ in range(len(q))]
        if self._use_gpu():
            return self.search_vectors_async(q, top_k, mmr).result()
        mat = self.matrix()
        qa = np.asarray(q.float().cpu().numpy() if isinstance(q, torch.Tensor) else q, dtype=np.float32)
        if qa.ndim == 1:
            qa = qa[None]
        out = []
        for qv in qa:
            if qv.shape[-1] != mat.shape[1]:
                scores = np.full(n, -1.0)
            else:
                prod = (mat * qv[None, :]).astype(np.float64).sum(1)
                na = float(np.sum((qv * qv).astype(np.float64)))
                nb = (mat * mat).astype(np.float64).sum(1)
                scores = prod / (np.sqrt(na) * np.sqrt(nb) + 1e-9)
            if mmr is None:
                order = np.argsort(-scores, kind="stable")[: min(k, n)]
            else:
                cand = np.argsort(-scores, kind="stable")[: min(pool, n)]
                order = [cand[p] for p, _, _ in mmr_select_f64(mat[cand], scores[cand], lam, k)]
            out.append([(int(j), float(scores[j])) for j in order])
        return out

    # ------------------------------------------------------------ lexical / hybrid
    def configure_lexical(self, hybrid_candidates: int = 24, rrf_k: int = 60, bm25_k1: float = 1.2,
                          bm25_b: float = 0.75):
        """RagConfig's hybrid-search settings; a changed k1 / b drops a built lexical index."""
        if (bm25_k1, bm25_b) != (self.bm25_k1, self.bm25_b):
            self._lex = None
        self.hybrid_candidates, self.rrf_k, self.bm25_k1, self.bm25_b = hybrid_candidates, rrf_k, bm25_k1, bm25_b

    def lexical(self):
        """The BM25 index over the chunk texts (:class:`.lexical.LexicalIndex`), built on first use
        under a lock and dropped by :meth:`add` / :meth:`load`: on the device when the vector
        search runs there, else on the host (the fp32 reference of ``ops.bm25_topk``)."""
        lex = self._lex
        if lex is None:
            from .lexical import LexicalIndex

            with self._lex_lock:
                lex = self._lex
                if lex is None:
                    dev = self.device if self.device.type == "cuda" and self._use_gpu() else torch.device("cpu")
                    lex = LexicalIndex([c.text for c in self.chunks], self.bm25_k1, self.bm25_b, dev)
                    self._lex = lex
        return lex

    def cosines(self, qv: np.ndarray, idx: Sequence[int]) -> list[float]:
        """Cosine of one query vector against the corpus rows ``idx`` (the hits that only the lexical
        list found): the arithmetic of the backend's scan -- float64 sums of f32 products on the
        exact backend, the bf16 rows with an fp32 dot on the GPU backend."""
        if not len(idx):
            return []
        if self._use_gpu():
            corpus, norms = self.gpu_tensors()
            if qv.shape[-1] != corpus.shape[1]:
                raise ValueError(f"query width {qv.shape[-1]} != corpus width {corpus.shape[1]}")
            ix = torch.as_tensor(list(idx), dtype=torch.long, device=corpus.device)
            q = torch.as_tensor(qv, dtype=torch.float32).to(torch.bfloat16).to(corpus.device).float().reshape(-1)
            dot = corpus[ix].float() @ q
            return (dot / (q.norm() * norms[ix] + 1e-9)).tolist()
        mat = self.matrix()[list(idx)]
        qv = np.asarray(qv, dtype=np.float32).reshape(-1)
        if qv.shape[-1] != mat.shape[1]:
            return [-1.0] * len(idx)
        prod = (mat * qv[None, :]).astype(np.float64).sum(1)
        na = float(np.sum((qv * qv).astype(np.float64)))
        nb = (mat * mat).astype(np.float64).sum(1)
        return (prod / (np.sqrt(na) * np.sqrt(nb) + 1e-9)).tolist()

    def _query_fused(self, query: str, k: int, take: int, mode: str, order_out: Optional[list] = None) -> list[RagHit]:
        """The best ``take`` chunks of the lexical order ('lexical') or of the reciprocal-rank fusion
        of the lexical and the cosine list ('hybrid'): fused(d) = sum over the lists holding d of
        1 / (rrf_k + rank), rank 1-based, sorted by fused descending, ties by lower chunk index."""
        if getattr(self, "_sharded", None) is not None:
            raise ValueError(f"mode '{mode}' is not supported with a sharded (tensor-parallel) corpus: use 'dense'")
        if not self.chunks:
            return []
        cn = min(64, max(k, int(self.hybrid_candidates)))
        qv = self.embedder.embed([query])
        with _tracer.span("rag.lexical", mode=mode, candidates=cn):
            lex = self.lexical().search([query], cn)[0]
        bm25 = dict(lex)
        cos: dict[int, float] = {}
        lists = [[d for d, _ in lex]]
        if mode == "hybrid":
            dense = self.search_vectors(qv, cn)[0]
            cos = dict(dense)
            lists.append([d for d, _ in dense])
        fused = rrf_fuse(lists, self.rrf_k)
        order = sorted(fused, key=lambda d: (-fused[d], d))[:take]
        if order_out is not None:  # the hits' chunk indices, for a later stage that needs the rows
            order_out.extend(order)
        missing = [d for d in order if d not in cos]
        cos.update(zip(missing, self.cosines(np.asarray(qv)[0], missing)))
        return [RagHit(self.chunks[d].id, self.chunks[d].source, self.chunks[d].text, float(cos[d]),
                       lexical_score=bm25.get(d), fused_score=fused[d]) for d in order]

    def _query_mmr(self, query: str, top_k: int, reranker, candidates: int, mode: str, lam: float,
                   mmr_candidates: int) -> list[RagHit]:
        """:meth:`query` with MMR as the last stage (docs/mmr.md): the earlier stages produce their
        order over a pool of ``min(64, max(top_k, mmr_candidates))`` hits, whose relevance is the
        cosine ('dense'), the rerank score (with a reranker) or ``fused_score * (rrf_k + 1) /
        n_lists`` ('hybrid' / 'lexical'); ``top_k`` of them are picked greedily."""
        if mode not in SEARCH_MODES:
            raise ValueError(f"mode must be one of {', '.join(SEARCH_MODES)} (got {mode!r})")
        lam = _check_mmr_lambda(lam)
        if getattr(self, "_sharded", None) is not None:
            raise ValueError(_SHARDED_MMR)
        k = max(1, top_k)
        pool = min(MMR_MAX_CANDIDATES, max(k, int(mmr_candidates)))
        take = pool if reranker is None else min(MMR_MAX_CANDIDATES, max(k, int(candidates), int(mmr_candidates)))
        idx: list[int] = []
        if mode != "dense":
            hits = self._query_fused(query, k, take, mode, idx)
            scale = (self.rrf_k + 1) / (2 if mode == "hybrid" else 1)
            rel = [h.fused_score * scale for h in hits]
        else:
            res = self.search_vectors(self.embedder.embed([query]), take)[0]
            idx = [j for j, _ in res]
            hits = self.hits(res)
            rel = [h.score for h in hits]
        if not hits:
            return hits
        if reranker is not None:
            rs = [float(s) for s in reranker.score(query, [h.text for h in hits])]
            if len(rs) != len(hits):
                raise ValueError(f"reranker returned {len(rs)} scores for {len(hits)} documents")
            order = sorted(range(len(hits)), key=lambda i: (-rs[i], i))[:pool]
            for i in order:
                hits[i].rerank_score = rs[i]
            hits, idx, rel = [hits[i] for i in order], [idx[i] for i in order], [rs[i] for i in order]
        else:
            hits, idx, rel = hits[:pool], idx[:pool], rel[:pool]
        kk = min(k, len(hits))
        with _tracer.span("rag.mmr", lam=lam, candidates=len(hits), k=kk):
            if self._use_gpu():
                corpus, norms = self.gpu_tensors()
                dev = corpus.device
                cid = torch.tensor([idx], dtype=torch.int32, device=dev)
                rl = torch.tensor([rel], dtype=torch.float32, device=dev)
                pos, _, _, mm, ms = ops.mmr_select(corpus, norms, cid, rl, lam, kk)
                picks = [(p, v, s) for p, v, s in zip(pos[0].tolist(), mm[0].tolist(), ms[0].tolist()) if p >= 0]
            else:
                picks = mmr_select_f64(self.matrix()[idx], rel, lam, kk)
        out = []
        for p, v, s in picks:
            hits[p].mmr_score, hits[p].max_sim = float(v), float(s)
            out.append(hits[p])
        return out

    def query(self, query: str, top_k: int = 5, reranker=None, candidates: int = 24, mode: str = "dense",
              mmr_lambda: Optional[float] = None, mmr_candidates: int = 24) -> list[RagHit]:
        """Top ``top_k`` hits by cosine.  With a ``reranker`` (``score(query, docs) -> floats``, see
        :mod:`.reranker`): ``max(top_k, candidates)`` cosine hits are scored by it and the best
        ``top_k`` come back in rerank order (ties by cosine rank); every hit keeps its cosine as
        ``score`` and carries the reranker's as ``rerank_score``.

        ``mode`` 'lexical' orders by BM25 and 'hybrid' by the reciprocal-rank fusion of the BM25 and
        the cosine list, ``min(64, max(top_k, hybrid_candidates))`` hits from each
        (docs/hybrid_search.md); the hits carry ``lexical_score`` and ``fused_score``, ``score`` stays
        the cosine, and a reranker scores the best ``max(top_k, candidates)`` of that order.  'dense'
        (the default) is the cosine scan alone.

        ``mmr_lambda`` in [0, 1] adds maximal-marginal-relevance selection as the last stage
        (docs/mmr.md) over the first ``min(64, max(top_k, mmr_candidates))`` hits of that order; the
        hits then carry ``mmr_score`` and ``max_sim``.  None (the default) is the path without it."""
        if mmr_lambda is not None:
            return self._query_mmr(query, top_k, reranker, candidates, mode, mmr_lambda, mmr_candidates)
        if mode not in SEARCH_MODES:
            raise ValueError(f"mode must be one of {', '.join(SEARCH_MODES)} (got {mode!r})")
        if mode != "dense":
            k = max(1, top_k)
            hits = self._query_fused(query, k, k if reranker is None else max(k, candidates), mode)
            if reranker is None or not hits:
                return hits
            top_k = k
        else:
            qv = self.embedder.embed([query])
            if reranker is None:
                return self.hits(self.search_vectors(qv, top_k)[0])
            hits = self.hits(self.search_vectors(qv, max(top_k, candidates))[0])
        if not hits:
            return hits
        rs = [float(s) for s in reranker.score(query, [h.text for h in hits])]
        if len(rs) != len(hits):
            raise ValueError(f"reranker returned {len(rs)} scores for {len(hits)} documents")
        order = sorted(range(len(hits)), key=lambda i: (-rs[i], i))[:top_k]
        out = []
        for i in order:
            hits[i].rerank_score = rs[i]
            out.append(hits[i])
        return out

    def query_batch(self, queries: Sequence[str], top_k: int = 5) -> list[list[RagHit]]:
        qv = self.embedder.embed(list(queries))
        return [self.hits(r) for r in self.search_vectors(qv, top_k)]

    def hits(self, res) -> list[RagHit]:
        return [RagHit(self.chunks[j].id, self.chunks[j].source, self.chunks[j].text, s) for j, s in res]

    # ------------------------------------------------------------ persistence
    def save(self, path: str):
        from safetensors.numpy import save_file

        p = Path(path)
        p.mkdir(parents=True, exist_ok=True)
        save_file({"embeddings": self.matrix().astype(np.float32)}, str(p / "embeddings.safetensors"))
        meta = {"chunks": [c.__dict__ for c in self.chunks], "file_hashes": self.file_hashes,
                "model": getattr(self.embedder, "model", None), "saved_at": time.time()}
        (p / "index.json").write_text(json.dumps(meta, ensure_ascii=False), encoding="utf-8")

    def load(self, path: str) -> bool:
        from safetensors.numpy import load_file

        p = Path(path)
        if not (p / "index.json").exists():
            return False
        meta = json.loads((p / "index.json").read_text(encoding="utf-8"))
        if meta.get("model") != getattr(self.embedder, "model", None):
            log.warning("[RAG] cached index built with %s, embedder is %s: ignoring cache",
                        meta.get("model"), getattr(self.embedder, "model", None))
            return False
        emb = load_file(str(p / "embeddings.safetensors"))["embeddings"]
        self.chunks = [RagChunk(**c) for c in meta["chunks"]]
        self._emb = list(emb)
        self._mat = emb if len(emb) else None
        self._gpu = None
        self._lex = None  # not persisted: rebuilt from the texts on demand
        self.file_hashes = meta.get("file_hashes", {})
        return True

    def build_incremental(self, folder: str, cache_dir: str, chunk_size: int = 800, overlap: int = 120) -> dict:
        """Load the cached index, re-embed only files whose content hash changed."""
        old = RagIndex(self.embedder, self.backend, str(self.device))
        have = old.load(cache_dir)
        files = enumerate_files(folder) if os.path.isdir(folder) else []
        reused = embedded = 0
        self.chunks, self._emb, self.file_hashes = [], [], {}
        by_src: dict[str, list[int]] = {}
        if have:
            for j, c in enumerate(old.chunks):
                by_src.setdefault(c.source, []).append(j)
        for path in files:
            raw = open(path, "rb").read()
            h = hashlib.sha256(raw).hexdigest()
            self.file_hashes[path] = h
            if have and old.file_hashes.get(path) == h and path in by_src:
                for j in by_src[path]:
                    self.chunks.append(old.chunks[j])
                    self._emb.append(old._emb[j])
                reused += len(by_src[path])
                continue
            text = raw.decode("utf-8", errors="replace").lstrip("﻿")
            chunks = chunk_document(text, chunk_size, overlap)
            name = os.path.basename(path)
            if chunks:
                self.add([f"{name}#{i}" for i in range(len(chunks))], [path] * len(chunks), chunks,
                         self.embedder.embed(chunks))
            embedded += len(chunks)
        self._mat = None
        self._gpu = None
        self._lex = None
        self.save(cache_dir)
        return {"reused": reused, "embedded": embedded, "total": len(self.chunks)}


__all__ = ["RagIndex", "RagChunk", "RagHit", "cosine_exact", "rrf_fuse", "enumerate_files", "split_by_markdown_headers",
           "chunk_sliding", "sanitize", "is_blank"]


def _rows(s, i, k):
    return [[(ii, ss) for ss, ii in zip(sr, ir) if ii >= 0][:k] for sr, ir in zip(s, i)]


class PendingSearch:
    """A launched :meth:`RagIndex.search_vectors_async`: ``ready()`` polls its event,
    ``result()`` waits for it (not for the device) and decodes the rows once."""

    def __init__(self, host=None, event=None, done=None):
        self._host, self._event, self._done = host, event, done
        self.wait_s = 0.0  # host time spent blocked in result()

    def ready(self) -> bool:
        return self._done is not None or self._event is None or self._event.query()

    def result(self) -> list:
        if self._done is None:
            t0 = time.perf_counter()
            if self._event is not None:
                self._event.synchronize()
            self.wait_s = time.perf_counter() - t0
            hs, hi, k = self._host
            self._done = _rows(hs.tolist(), hi.tolist(), k)
            M.KNN_LAT.observe(self.wait_s)
        return self._done
