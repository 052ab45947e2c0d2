"""Batched cross-encoder scoring (the ``/v1/rerank`` compute).

A query and its candidate documents are tokenised into ``[CLS] q [SEP] d [SEP]`` pairs (the
query once per call), packed varlen into micro-batches under the embedding engine's token budget
(the type ids travel with the ids) and run through a :class:`CrossEncoderModel`; one f32 score
per pair comes back.  Each pair's score depends only on its own rows, so the micro-batch split
never changes a score.  No hipGraphs: every call is a handful of eager launches on the caller's
stream (``score``) or on one of the engine's high-priority streams (``score_cpu``).
"""
from __future__ import annotations

import time

import numpy as np
import torch

from ..utils import metrics as M
from .embed_engine import EMBED_STREAMS, EmbeddingEngine


class RerankEngine(EmbeddingEngine):
    def encode(self, query: str, docs: list[str]) -> tuple[list[list[int]], list[list[int]]]:
        """(ids, type_ids) of the pairs, truncated to the engine's max length."""
        return self.tok.encode_pairs(query, list(docs), self.max_len)

    @torch.inference_mode()
    def score_ids(self, ids: list[list[int]], types: list[list[int]], activation: int = 0) -> torch.Tensor:
        """Scores of already tokenised pairs: f32 [n] on the engine's device, launched
        asynchronously on the current stream in token-budgeted varlen micro-batches."""
        d = self.device
        out = torch.empty((len(ids),), dtype=torch.float32, device=d)
        if not ids:
            return out
        flat, lens = self._flat(ids)
        tflat, _ = self._flat_types(types)
        starts = np.zeros(len(lens) + 1, dtype=np.int64)
        starts[1:] = np.cumsum(lens)
        i = 0
        while i < len(lens):
            j = i + 1
            while j < len(lens) and starts[j + 1] - starts[i] <= self.budget:
                j += 1
            a, b = int(starts[i]), int(starts[j])
            ln = lens[i:j]
            pos = (np.arange(b - a, dtype=np.int64) - np.repeat(starts[i:j] - a, ln)).astype(np.int32)
            cu = (starts[i:j + 1] - a).astype(np.int32)
            s = self.model(torch.from_numpy(flat[a:b]).to(d, non_blocking=True),
                           torch.from_numpy(cu).to(d, non_blocking=True),
                           torch.from_numpy(pos).to(d, non_blocking=True), ln.tolist(),
                           type_ids=torch.from_numpy(tflat[a:b]).to(d, non_blocking=True),
                           activation=int(activation))
            if j - i == len(lens):  # one micro-batch: the kernel's output is the result
                return s
            out[i:j].copy_(s)
            i = j
        return out

    @staticmethod
    def _flat_types(types) -> tuple[np.ndarray, int]:
        n = sum(map(len, types))
        flat = np.fromiter((t for s in types for t in s), dtype=np.int32, count=n)
        return flat, n

    def score(self, query: str, docs: list[str], activation: int = 0) -> torch.Tensor:
        """f32 [n] scores of (query, doc) pairs on the device (0: logits, 1: sigmoid)."""
        t0 = time.perf_counter()
        ids, types = self.encode(query, docs)
        with self.lock:
            r = self.score_ids(ids, types, activation)
        M.EMBED_LAT.observe(time.perf_counter() - t0)
        return r

    def score_cpu(self, query: str, docs: list[str], activation: int = 0, return_tokens: bool = False):
        """Host numpy f32 [n] scores (with ``return_tokens``: also the number of tokens encoded).
        On the GPU the launches go on one of this engine's high-priority streams under the lock;
        the wait for the copy happens outside it, as in ``embed_cpu``."""
        t0 = time.perf_counter()
        ids, types = self.encode(query, docs)
        ntok = sum(map(len, ids))
        if self.device.type != "cuda":
            with self.lock:
                arr = self.score_ids(ids, types, activation).numpy().copy()
        else:
            with self.lock:
                if getattr(self, "_streams", None) is None:
                    self._streams = [torch.cuda.Stream(self.device, priority=-1) for _ in range(EMBED_STREAMS)]
                    self._next = 0
                st = self._streams[self._next]
                self._next = (self._next + 1) % len(self._streams)
                with torch.cuda.stream(st):
                    r = self.score_ids(ids, types, activation)
                    host = torch.empty(r.shape, dtype=torch.float32, pin_memory=True)
                    host.copy_(r, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(st)
            ev.synchronize()
            arr = host.numpy().copy()
        M.EMBED_LAT.observe(time.perf_counter() - t0)
        return (arr, ntok) if return_tokens else arr
