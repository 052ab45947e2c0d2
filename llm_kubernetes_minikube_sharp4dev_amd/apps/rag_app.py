"""Port of the ``Minimal_RAG`` service (``Minimal_RAG/Program.cs``) with identical routes
and JSON contracts:

  GET  /health       -> {"status":"ok"}                                  (C2, :55)
  POST /rag/search   pure retrieval, topK default 5 clamp [1,10], best-score
                     0.20 floor, 260-char previews                        (C3, :62-100);
                     optional "mode": dense | lexical | hybrid (docs/hybrid_search.md);
                     optional "mmrLambda": MMR selection as the last stage (docs/mmr.md)
  POST /agent_rag    retrieve top-6 -> citations -> LLM tool call -> gated k8s
                     action -> {result, citations, note}                  (C4, :106-316)

Bootstrap (C1): the index is built from ``knowledge_dir`` BEFORE serving
(``Program.cs:50``), constants come from :class:`~..config.Config`.  The LLM and the
embedder are pluggable: HTTP to an Ollama-compatible server (as the reference), or
in-process MI355X engines.
"""
from __future__ import annotations

from fastapi import Request  # module level: FastAPI resolves string annotations here

import asyncio
import time
from typing import Optional

from ..agent.dotnet_json import _num as net_num
from ..agent.json_extract import extract_json_object
from ..agent.policy import select_citations
from ..agent.prompts import RAG_AGENT_SYSTEM, json_prompt, rag_agent_input
from ..agent.tools import dispatch_rag_tool
from ..config import SEARCH_MODES, Config, mmr_lambda_ok, validate_mmr
from ..rag.chunking import is_blank, u16len, u16slice
from ..utils import metrics as M
from ..utils.logging import get_logger
from ..utils.tracing import Tracer
from .common import BindError, NetJSONResponse, add_https_redirection, bind_body, member, respond

log = get_logger("RAG.Search")


def create_rag_app(cfg: Optional[Config] = None, index=None, llm=None, k8s=None, build_index: bool = True,
                   reranker=None):
    """``reranker``: the second stage of /rag/search (``score(query, docs)``, :mod:`..rag.reranker`),
    used only when ``cfg.rag.rerank_model`` is set."""
    from fastapi import FastAPI, Request
    from starlette.responses import Response

    cfg = cfg or Config()
    r = cfg.rag
    app = FastAPI(title="Minimal_RAG (MI355X)")
    app.state.cfg, app.state.index, app.state.llm, app.state.k8s = cfg, index, llm, k8s
    if r.rerank_model and reranker is None:
        raise ValueError(f"rag.rerank_model is '{r.rerank_model}' but no reranker was given to the RAG app")
    app.state.reranker = reranker if r.rerank_model else None
    if r.search_mode not in SEARCH_MODES:
        raise ValueError(f"rag.search_mode must be one of {', '.join(SEARCH_MODES)} (got '{r.search_mode}')")
    validate_mmr(r)
    agent_mmr = None if r.agent_mmr_lambda is None else (r.agent_mmr_lambda, r.mmr_candidates)
    tracer = Tracer("rag_app")
    app.state.tracer = tracer
    if build_index and index is not None and len(index) == 0:
        if r.cache_dir:
            index.build_incremental(r.knowledge_dir, r.cache_dir, r.chunk_size, r.chunk_overlap)
        else:
            index.build_from_folder(r.knowledge_dir, r.chunk_size, r.chunk_overlap)
    if hasattr(index, "configure_lexical"):
        index.configure_lexical(r.hybrid_candidates, r.rrf_k, r.bm25_k1, r.bm25_b)
        if r.search_mode != "dense" and len(index):
            index.lexical()  # at start-up, not on the first query
    if cfg.server.https_redirection:
        add_https_redirection(app, cfg.server.rag_https_port)

    import numpy as np

    from ..serving.batcher import MicroBatcher

    # the app's kNN shares the GPU with the model server's engine: its few small kernels go on a
    # high-priority stream so they are dispatched ahead of the engine's queued step kernels
    knn_stream = None
    if getattr(getattr(index, "device", None), "type", "cpu") == "cuda":
        import torch

        knn_stream = torch.cuda.Stream(index.device, priority=-1)

    def knn_batch(qs):
        qa = np.stack([np.asarray(q, dtype=np.float32) for q in qs])
        kw = {} if agent_mmr is None else {"mmr": agent_mmr}  # opt-in (docs/mmr.md)
        if knn_stream is None:
            return index.search_vectors(qa, r.agent_topk, **kw)
        import torch

        with torch.cuda.stream(knn_stream):
            return index.search_vectors(qa, r.agent_topk, **kw)

    knn_batcher = MicroBatcher(knn_batch, max_items=64)

    @app.get("/health")
    async def health():
        return NetJSONResponse({"status": "ok"})

    def _rr(h) -> dict:  # (absent in mode 'dense' / without a reranker: the response is unchanged)
        out = {}
        if getattr(h, "fused_score", None) is not None:
            out = {"lexicalScore": h.lexical_score, "fusedScore": h.fused_score}
        rs = getattr(h, "rerank_score", None)
        if rs is not None:
            out = {**out, "rerankScore": rs}
        if getattr(h, "mmr_score", None) is not None:
            out = {**out, "mmrScore": h.mmr_score, "maxSim": h.max_sim}
        return out

    @app.post("/rag/search")
    async def rag_search(request: Request):
        t0 = time.perf_counter()
        try:
            body = await bind_body(request)
            query = member(body, "query")
            top_k = member(body, "topK", "int")
        except BindError:
            return Response(status_code=400)
        mode = None
        lam, lam_given = None, False
        for key, val in body.items():  # case-insensitive, like member()
            if key.lower() == "mode":
                mode = val
            elif key.lower() == "mmrlambda":
                lam, lam_given = val, True
        if not lam_given:
            lam = r.mmr_lambda
        elif lam is not None and not mmr_lambda_ok(lam):
            return NetJSONResponse({"error": "mmrLambda must be a number between 0 and 1"}, status_code=400)
        if mode is None:
            mode = r.search_mode
        if not isinstance(mode, str) or mode not in SEARCH_MODES:
            return NetJSONResponse({"error": f"mode must be one of {', '.join(SEARCH_MODES)}"}, status_code=400)
        if is_blank(query):
            return NetJSONResponse({"error": "Query vuota"}, status_code=400)
        k = r.search_default_topk if top_k is None else min(max(top_k, r.search_topk_min), r.search_topk_max)
        with tracer.span("rag.search", k=k):
            if lam is not None:  # opt-in last stage: MMR over the order of the stages before it
                try:
                    hits = await asyncio.to_thread(index.query, query, k, app.state.reranker, r.rerank_candidates, mode,
                                                   float(lam), r.mmr_candidates)
                except ValueError as e:  # a sharded corpus serves neither MMR nor the non-dense modes
                    return NetJSONResponse({"error": f"{e}"}, status_code=400)
            elif mode != "dense":  # opt-in first stage: BM25 alone, or fused with the cosine list
                try:
                    hits = await asyncio.to_thread(index.query, query, k, app.state.reranker, r.rerank_candidates, mode)
                except ValueError as e:  # a sharded corpus serves 'dense' only
                    return NetJSONResponse({"error": f"mode: {e}"}, status_code=400)
            elif app.state.reranker is None:
                hits = await asyncio.to_thread(index.query, query, k)
            else:  # opt-in second stage: the best k of the cosine candidates, in rerank order
                hits = await asyncio.to_thread(index.query, query, k, app.state.reranker, r.rerank_candidates)
        if not hits:
            return NetJSONResponse({"info": "Nessun risultato. L'indice potrebbe essere vuoto.", "results": []})
        best = max(h.score for h in hits)
        log.info("[RAG] Best score = %s", best)
        M.HTTP_LAT.labels("/rag/search").observe(time.perf_counter() - t0)
        if best < r.search_min_score:
            return NetJSONResponse({
                "info": f"Best score basso ({net_num(best)}). Aggiungi runbook più pertinenti o verifica l'indice.",
                "results": [{"id": h.id, "source": h.source, "score": h.score, **_rr(h)} for h in hits]})
        out = []
        for h in hits:
            prev = u16slice(h.text, 0, r.preview_chars) + "..." if u16len(h.text) > r.preview_chars else h.text
            out.append({"id": h.id, "source": h.source, "score": h.score, **_rr(h), "preview": prev})
        return NetJSONResponse(out)

    @app.post("/agent_rag")
    async def agent_rag(request: Request):
        t0 = time.perf_counter()
        try:
            body = await bind_body(request)
            prompt = member(body, "prompt")
        except BindError:
            return Response(status_code=400)
        if is_blank(prompt):
            return NetJSONResponse({"error": "Prompt mancante"}, status_code=400)
        with tracer.span("rag.retrieve"):
            if hasattr(index, "search_vectors") and hasattr(index, "embedder"):
                with tracer.span("rag.embed"):
                    if hasattr(index.embedder, "aembed_one"):  # HTTP embedder: no worker thread
                        qv = (await index.embedder.aembed_one(prompt))[None]
                    else:
                        qv = await asyncio.to_thread(index.embedder.embed, [prompt])
                with tracer.span("rag.knn"):
                    # concurrent requests' queries share one kNN launch (one corpus pass)
                    res = await knn_batcher.submit([qv[0]])
                hits = index.hits(res[0])
            else:
                hits = await asyncio.to_thread(index.query, prompt, r.agent_topk)
        if not hits:
            return NetJSONResponse({"result": None, "citations": [], "note": "Nessuna evidenza trovata nei runbook."})
        citations, evidence = select_citations(hits, r.evidence_min_score, r.citation_best_ratio)
        full = json_prompt(RAG_AGENT_SYSTEM, rag_agent_input(prompt, evidence, r.evidence_text_chars))
        with tracer.span("llm.generate", prompt_chars=len(full)):
            raw = await app.state.llm.generate(full)
        tool_json = extract_json_object(raw)
        with tracer.span("agent.dispatch"):
            status, out = await asyncio.to_thread(dispatch_rag_tool, app.state.k8s, tool_json, citations, evidence, cfg)
        M.HTTP_LAT.labels("/agent_rag").observe(time.perf_counter() - t0)
        return respond(status, out)

    @app.get("/debug/spans")
    async def spans(since: float = 0.0):
        """Per-span latency summary (count / mean / p50 / p99) since a time.time() stamp."""
        from ..utils import tracing

        return NetJSONResponse(tracing.summary(since))

    @app.get("/metrics")
    async def metrics():
        return Response(M.render(), media_type="text/plain; version=0.0.4")

    return app
