"""Device cost of the cross-encoder score head (docs/rerank.md):

    python benchmarks/rerank_cost.py            # every case below, one JSON line each

* ``lk_rerank_head`` against the chain of framework ops it replaces (index_select -> F.linear ->
  tanh -> matvec -> sigmoid) at H 384 / 768 and B 24 / 256, on the same bf16 inputs;
* the head as a share of a whole ``ms-marco-minilm-l6`` pass over 24 pairs of 256 tokens.

Timed with device events by the protocol of docs/sampling.md: "per call" is ``--calls`` calls, each
between its own event pair (median and minimum); "burst" is ``--burst`` back-to-back calls between
one event pair, so the device never waits for the host."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

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
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--burst", type=int, default=500)
    ap.add_argument("--pass-calls", type=int, default=30)
    ap.add_argument("--pass-burst", type=int, default=30)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F

    from llm_kubernetes_minikube_sharp4dev_amd import ops
    from llm_kubernetes_minikube_sharp4dev_amd.models import build_reranker

    dev = torch.device("cuda", 0)
    # the floor of every figure below: one launch of a one-wave kernel that does nothing
    from llm_kubernetes_minikube_sharp4dev_amd.ops import _ext

    print(json.dumps({"case": "launch_floor", "kernel": "lk_window_mark",
                      **timed(torch, lambda: _ext.lib().window_mark(0), a.calls, a.burst)}), flush=True)
    g = torch.Generator().manual_seed(0)
    for H in (384, 768):
        for B in (24, 256):
            L = 256
            hidden = torch.randn(B * L, H, generator=g).to(torch.bfloat16).to(dev)
            cu = (torch.arange(B + 1, dtype=torch.int32) * L).to(dev)
            first = cu[:-1].long()
            pw = (torch.randn(H, H, generator=g) * 0.05).to(torch.bfloat16).to(dev)
            pb = (torch.randn(H, generator=g) * 0.02).to(torch.bfloat16).to(dev)
            cw = (torch.randn(1, H, generator=g) * 0.05).to(torch.bfloat16).to(dev)
            cb = torch.zeros(1, dtype=torch.bfloat16, device=dev)

            def kernel():
                return ops.rerank_head(hidden, cu, pw, pb, cw, cb, 1)

            def chain():
                x = hidden.index_select(0, first)
                t = torch.tanh(F.linear(x, pw, pb))
                return torch.sigmoid(F.linear(t, cw, cb).float().squeeze(-1))

            diff = float((kernel() - chain()).abs().max())
            print(json.dumps({"case": "head", "H": H, "B": B, "kernel": timed(torch, kernel, a.calls, a.burst),
                              "framework_chain": timed(torch, chain, a.calls, a.burst),
                              "max_abs_diff_vs_bf16_chain": round(diff, 5)}), flush=True)

    # the head's share of a whole pass: 24 pairs of 256 tokens through ms-marco-minilm-l6
    m = build_reranker("ms-marco-minilm-l6", device=dev)
    B, L = 24, 256
    V = m.cfg.vocab_size
    ids = torch.randint(1000, V, (B * L,), generator=g).int().to(dev)
    types = (torch.arange(B * L) % L >= 24).int().to(dev)
    pos = (torch.arange(B * L) % L).int().to(dev)
    cu = (torch.arange(B + 1, dtype=torch.int32) * L).to(dev)
    lens = [L] * B
    G = 1
    ts, tq = ops.prefill_tiles(lens, lens, G, False, m.D)
    tiles = (torch.from_numpy(ts).to(dev), torch.from_numpy(tq).to(dev))
    with torch.inference_mode():
        h = super(type(m), m).forward(ids, cu, pos, lens, type_ids=types, pool=False, tiles=tiles)

        def whole():
            return m(ids, cu, pos, lens, type_ids=types, activation=1, tiles=tiles)

        def head():
            return ops.rerank_head(h, cu, m.pool_w, m.pool_b, m.cls_w, m.cls_b, 1)

        tw = timed(torch, whole, a.pass_calls, a.pass_burst)
        th = timed(torch, head, a.calls, a.burst)
    print(json.dumps({"case": "pass", "model": "ms-marco-minilm-l6", "pairs": B, "tokens_per_pair": L, "whole_pass": tw,
                      "head": th, "head_share_of_burst_pct": round(100.0 * th["burst_us"] / tw["burst_us"], 3)}), flush=True)


if __name__ == "__main__":
    main()
