"""Cost of the MMR selection next to the dense scan on the synthetic runbook corpus (docs/mmr.md):

    python benchmarks/mmr_cost.py                 # 100k documents (~485k chunks), one JSON line per case
    python benchmarks/mmr_cost.py --docs 2000     # a rehearsal size

* ``ops.mmr_select`` at (C, K) = (24, 6) and (64, 10) for nq 1 and 32 queries of ``make_queries``, the
  candidates and their relevance taken from a real ``ops.knn_topk`` of width C;
* next to it, in the same process, ``ops.knn_topk`` at K = 6 (today's /agent_rag retrieval) and K = 24
  (the scan in front of MMR), and the chain ``knn_topk(24)`` + ``mmr_select(24, 6)`` as RagIndex issues
  it, so that the chain can be read against today's ``knn_topk(6)``.

"per call" is ``--calls`` calls, each between its own event pair (median and minimum); "burst" is
``--burst`` back-to-back calls between one event pair (the protocol of benchmarks/bm25_cost.py).  The
dense vectors come from the ``--embed`` encoder preset (D = 768) with seeded random weights, as in
bench.py's index."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.bm25_cost import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--burst", type=int, default=500)
    ap.add_argument("--embed", default="bge-base")
    ap.add_argument("--lam", type=float, default=0.5)
    a = ap.parse_args()
    import torch

    from llm_kubernetes_minikube_sharp4dev_amd import ops
    from llm_kubernetes_minikube_sharp4dev_amd.engine.embed_engine import EmbeddingEngine
    from llm_kubernetes_minikube_sharp4dev_amd.models import build_encoder
    from llm_kubernetes_minikube_sharp4dev_amd.models.tokenizer import builtin_tokenizer
    from llm_kubernetes_minikube_sharp4dev_amd.ops import _ext
    from llm_kubernetes_minikube_sharp4dev_amd.rag.corpus import build_chunks
    from llm_kubernetes_minikube_sharp4dev_amd.rag.synthetic import make_queries

    assert torch.cuda.is_available(), "mmr_cost.py measures on the GPU"
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    texts = [c[2] for c in build_chunks(a.docs, 0, workers=8)]
    enc = build_encoder(a.embed, device=dev, seed=0, dtype=torch.bfloat16)
    eng = EmbeddingEngine(enc, builtin_tokenizer(), name=a.embed, max_tokens_per_batch=131072)
    corpus = eng.embed(texts).to(torch.bfloat16).contiguous()
    cnorm = ops.row_norms(corpus)
    torch.cuda.synchronize()
    print(json.dumps({"case": "corpus", "docs": a.docs, "chunks": len(texts), "D": corpus.shape[1], "embed": a.embed,
                      "wall_s": round(time.perf_counter() - t0, 2)}), flush=True)
    print(json.dumps({"case": "launch_floor", "kernel": "lk_window_mark",
                      **timed(torch, lambda: _ext.lib().window_mark(0), a.calls, a.burst)}), flush=True)

    for nq in (1, 32):
        qv = eng.embed(make_queries(nq, seed=1)).to(torch.bfloat16).contiguous()
        qn = ops.row_norms(qv)
        row = {"case": "mmr", "nq": nq, "lam": a.lam}
        for K in (6, 24):
            row[f"knn_topk_{K}"] = timed(torch, lambda: ops.knn_topk(corpus, cnorm, qv, qn, K), a.calls, a.burst)
        for C, K in ((24, 6), (64, 10)):
            rel, cid = ops.knn_topk(corpus, cnorm, qv, qn, C)
            out = ops.mmr_select(corpus, cnorm, cid, rel, a.lam, K)
            moved = int((out[0] != torch.arange(K, device=dev)[None, :]).any(dim=1).sum())
            row[f"mmr_select_{C}_{K}"] = {**timed(torch, lambda: ops.mmr_select(corpus, cnorm, cid, rel, a.lam, K),
                                                  a.calls, a.burst), "queries_reordered": moved}

        def chain():
            s, i = ops.knn_topk(corpus, cnorm, qv, qn, 24)
            return ops.mmr_select(corpus, cnorm, i, s, a.lam, 6)

        row["knn_topk_24_then_mmr_select_24_6"] = timed(torch, chain, a.calls, a.burst)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
