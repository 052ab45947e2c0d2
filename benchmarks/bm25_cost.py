"""Cost of the lexical side of hybrid search on the synthetic runbook corpus (docs/hybrid_search.md):

    python benchmarks/bm25_cost.py                 # 100k documents (~485k chunks), one JSON line per case
    python benchmarks/bm25_cost.py --docs 2000     # a rehearsal size

* the lexical index build: wall time, device bytes, N / V / nnz;
* ``ops.bm25_topk`` against ``ops.knn_topk`` (the dense scan, bf16 corpus of the same chunks) for
  nq 1 and 32 queries of ``make_queries``, K = the serving default of 24 candidates: "per call" is
  ``--calls`` calls, each between its own event pair (median and minimum); "burst" is ``--burst``
  back-to-back calls between one event pair (the protocol of benchmarks/rerank_cost.py).  The
  BM25 call is the op as RagIndex makes it: q_ptr checked on the host and copied, two launches;
* sum of df over a query's terms (the postings the kernel scans): mean and max;
* recall@6 of dense, lexical and hybrid (RRF of 24 + 24 candidates), counted per document.  The
  synthetic queries have no labelled answer, so a query's target is the document of the chunk the
  dense scan ranks first (dense recall on that set is 1 by construction); the second set replaces
  each query with the rarest term of its target document (the number in a front matter's title
  and slug where the document has one).  A description of the corpus, not a gate.

The dense vectors come from the ``--embed`` encoder preset with seeded random weights, as in
bench.py's index."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, call, calls, burst):
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    per = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(burst):
        call()
    e1.record()
    e1.synchronize()
    return {"per_call_us_median": round(statistics.median(per), 2), "per_call_us_min": round(min(per), 2),
            "burst_us": round(e0.elapsed_time(e1) * 1e3 / burst, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--burst", type=int, default=500)
    ap.add_argument("--queries", type=int, default=256, help="queries of the df and recall statistics")
    ap.add_argument("--embed", default="bge-base")
    ap.add_argument("--k", type=int, default=24)
    a = ap.parse_args()
    import numpy as np
    import torch

    from llm_kubernetes_minikube_sharp4dev_amd import ops
    from llm_kubernetes_minikube_sharp4dev_amd.engine.embed_engine import EmbeddingEngine
    from llm_kubernetes_minikube_sharp4dev_amd.models import build_encoder
    from llm_kubernetes_minikube_sharp4dev_amd.models.tokenizer import builtin_tokenizer
    from llm_kubernetes_minikube_sharp4dev_amd.ops import _ext
    from llm_kubernetes_minikube_sharp4dev_amd.rag.corpus import build_chunks
    from llm_kubernetes_minikube_sharp4dev_amd.rag.index import rrf_fuse
    from llm_kubernetes_minikube_sharp4dev_amd.rag.lexical import LexicalIndex, analyse
    from llm_kubernetes_minikube_sharp4dev_amd.rag.synthetic import make_queries

    assert torch.cuda.is_available(), "bm25_cost.py measures on the GPU"
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    chunks = build_chunks(a.docs, 0, workers=8)
    texts = [c[2] for c in chunks]
    print(json.dumps({"case": "corpus", "docs": a.docs, "chunks": len(texts), "wall_s": round(time.perf_counter() - t0, 2)}),
          flush=True)

    lex = LexicalIndex(texts, device=dev)
    torch.cuda.synchronize()
    print(json.dumps({"case": "lexical_build", "wall_s": round(lex.build_s, 2), "device_bytes": lex.nbytes, "N": lex.N,
                      "V": lex.V, "nnz": lex.nnz, "avgdl": round(lex.avgdl, 2)}), flush=True)

    t0 = time.perf_counter()
    enc = build_encoder(a.embed, device=dev, seed=0, dtype=torch.bfloat16)
    eng = EmbeddingEngine(enc, builtin_tokenizer(), name=a.embed, max_tokens_per_batch=131072)
    corpus = eng.embed(texts).to(torch.bfloat16).contiguous()
    cnorm = ops.row_norms(corpus)
    torch.cuda.synchronize()
    print(json.dumps({"case": "dense_build", "embed": a.embed, "wall_s": round(time.perf_counter() - t0, 2),
                      "device_bytes": corpus.numel() * 2 + cnorm.numel() * 4}), flush=True)

    print(json.dumps({"case": "launch_floor", "kernel": "lk_window_mark",
                      **timed(torch, lambda: _ext.lib().window_mark(0), a.calls, a.burst)}), flush=True)
    for nq in (1, 32):
        qs = make_queries(nq, seed=1)
        t0 = time.perf_counter()
        for _ in range(20):
            q_ptr, q_term, q_w = lex.encode(qs)
        encode_us = (time.perf_counter() - t0) / 20 * 1e6
        qt, qw = q_term.to(dev), q_w.to(dev)
        qv = eng.embed(qs).to(torch.bfloat16).contiguous()
        qn = ops.row_norms(qv)

        def bm25():
            return ops.bm25_topk(lex.term_ptr, lex.post_doc, lex.post_tf, lex.kn, q_ptr, qt, qw, a.k)

        def knn():
            return ops.knn_topk(corpus, cnorm, qv, qn, a.k)

        sum_df = [lex.sum_df(q) for q in qs]
        print(json.dumps({"case": "topk", "nq": nq, "K": a.k, "terms": int(q_ptr[-1]), "sum_df": int(sum(sum_df)),
                          "host_encode_us": round(encode_us, 1), "bm25_topk": timed(torch, bm25, a.calls, a.burst),
                          "knn_topk": timed(torch, knn, a.calls, a.burst)}), flush=True)

    qs = make_queries(a.queries, seed=2)
    sdf = [lex.sum_df(q) for q in qs]
    print(json.dumps({"case": "sum_df", "queries": len(qs), "mean": round(float(np.mean(sdf)), 1), "max": int(max(sdf)),
                      "terms_mean": round(float(np.mean([len(lex.encode_one(q)[0]) for q in qs])), 2)}), flush=True)

    def dense_lists(queries, k):
        out = []
        for lo in range(0, len(queries), 32):
            qv = eng.embed(queries[lo:lo + 32]).to(torch.bfloat16).contiguous()
            _, i = ops.knn_topk(corpus, cnorm, qv, ops.row_norms(qv), k)
            out += [[d for d in row if d >= 0] for row in i.tolist()]
        return out

    def lexical_lists(queries, k):
        out = []
        for lo in range(0, len(queries), 32):
            out += [[d for d, _ in row] for row in lex.search(queries[lo:lo + 32], k)]
        return out

    # recall is counted per document: a hit is any of the best six chunks from the target's document
    doc_of = [c[1] for c in chunks]
    by_doc: dict = {}
    for j, src in enumerate(doc_of):
        by_doc.setdefault(src, []).append(j)

    def recall(queries, targets, name):
        dl, ll = dense_lists(queries, a.k), lexical_lists(queries, a.k)
        hyb = []
        for d, l in zip(dl, ll):
            f = rrf_fuse([l, d], 60)
            hyb.append(sorted(f, key=lambda x: (-f[x], x))[:6])
        r = lambda lists: round(sum(any(doc_of[j] == doc_of[t] for j in row[:6])  # noqa: E731
                                    for t, row in zip(targets, lists)) / len(targets), 4)
        print(json.dumps({"case": "recall_at_6", "set": name, "queries": len(queries), "dense": r(dl), "lexical": r(ll),
                          "hybrid": r(hyb), "lexical_empty": sum(not row for row in ll)}), flush=True)

    targets = [row[0] for row in dense_lists(qs, 1)]
    recall(qs, targets, "make_queries (target = the document of the dense top-1 chunk)")
    rare = []
    for t in targets:
        terms = {x for j in by_doc[doc_of[t]] for x in analyse(texts[j]) if len(x) >= 4}
        rare.append(min(terms, key=lambda x: (int(lex.df[lex.term_id[x]]), x)))
    df_rare = [int(lex.df[lex.term_id[x]]) for x in rare]
    print(json.dumps({"case": "rare_identifier", "examples": rare[:5], "df_median": int(np.median(df_rare)),
                      "df_max": int(max(df_rare)), "df_le_2": sum(d <= 2 for d in df_rare)}), flush=True)
    recall(rare, targets, "rarest term (>= 4 characters) of the target document")

if __name__ == "__main__":
    main()
