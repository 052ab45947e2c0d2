"""Second-stage rerankers for ``RagIndex.query(..., reranker=...)``: an object with
``score(query, docs) -> sequence of float`` (higher = more relevant).

* :class:`LocalReranker` — in-process cross-encoder (:class:`~..engine.rerank_engine.RerankEngine`);
  the score is the sigmoid of the pair's logit, as ``POST /v1/rerank`` reports it.
* :class:`HttpReranker` — ``POST /v1/rerank`` of an Ollama/OpenAI-compatible server.
"""
from __future__ import annotations

import json
from typing import Sequence

import numpy as np


class RerankError(RuntimeError):
    pass


class LocalReranker:
    def __init__(self, engine):
        self.engine = engine
        self.model = engine.name

    def score(self, query: str, docs: Sequence[str]) -> np.ndarray:
        return np.asarray(self.engine.score_cpu(query, list(docs), 1), dtype=np.float32)


class HttpReranker:
    def __init__(self, base_url: str = "http://localhost:11434", model: str = "ms-marco-minilm-l6",
                 client=None, timeout: float = 120.0):
        import httpx

        self.model = model
        self.client = client or httpx.Client(base_url=base_url, timeout=timeout)

    def score(self, query: str, docs: Sequence[str]) -> np.ndarray:
        docs = list(docs)
        out = np.zeros(len(docs), np.float32)
        if not docs:
            return out
        payload = {"model": self.model, "query": query, "documents": docs}
        r = self.client.post("/v1/rerank", content=json.dumps(payload, ensure_ascii=False).encode("utf-8"),
                             headers={"Content-Type": "application/json; charset=utf-8"})
        if not (200 <= r.status_code < 300):
            raise RerankError(f"/v1/rerank answered {r.status_code}")
        res = r.json().get("results", [])
        if sorted(x.get("index") for x in res) != list(range(len(docs))):
            raise RerankError("/v1/rerank did not score every document")
        for x in res:
            out[x["index"]] = float(x["relevance_score"])
        return out
