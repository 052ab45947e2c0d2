"""Device cost of constraining one step's logits (docs/structured_outputs.md), one arm per process:

    python benchmarks/mask_cost.py --arm mask     # pool of bitmasks + one lk_mask_logits launch
    python benchmarks/mask_cost.py --arm dense    # the id-list path of a fused batch: full +
                                                  # index_fill_ + index_add_ + .float()
    python benchmarks/mask_cost.py --host         # host cost of a cold / cached grammar mask (CPU)

Both arms constrain the same B x V bf16 logits to the same allowed sets (8 distinct sets of
~100k ids, the size of a JSON-string state, cycled over the rows) and end with the f32 [B, V]
tensor the fused sampler reads.  "per call": each call between its own event pair; "burst":
back-to-back calls between one pair.  The dense arm also reports the wall time of the per-step
upload of its id lists (a pageable host-to-device copy), which the mask arm does not have.
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_cost():
    from llm_kubernetes_minikube_sharp4dev_amd.engine.schema_grammar import SchemaGrammar, _Pieces
    from llm_kubernetes_minikube_sharp4dev_amd.models.tokenizer import builtin_tokenizer

    tok = builtin_tokenizer()
    t0 = time.perf_counter()
    _Pieces.get(tok)
    tables_ms = (time.perf_counter() - t0) * 1e3
    schema = {"type": "object", "properties": {"action": {"enum": ["list_pods", "get_logs", "scale_deployment"]},
                                               "name": {"type": "string", "maxLength": 200}, "replicas": {"type": "integer"},
                                               "extra": {}}, "required": ["action", "name", "replicas", "extra"]}
    t0 = time.perf_counter()
    g = SchemaGrammar(tok, schema)
    compile_ms = (time.perf_counter() - t0) * 1e3
    out = {"tokenizer_vocab": tok.vocab_size, "piece_tables_ms": round(tables_ms, 1), "compile_ms": round(compile_ms, 2)}
    states = {"forced_key": "", "enum_choice": '{"action":"', "string_free": '{"action":"get_logs","name":"ab',
              "string_near_limit": '{"action":"get_logs","name":"' + "a" * 197, "integer": '{"action":"get_logs","name":"","replicas":1',
              "any_value_start": '{"action":"get_logs","name":"","replicas":1,"extra":',
              "any_value_string": '{"action":"get_logs","name":"","replicas":1,"extra":["x'}
    for name, text in states.items():
        st = g.feed_text(g.start, text)
        t0 = time.perf_counter()
        m = g.mask(st)
        cold = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for _ in range(1000):
            g.mask(st)
        cached = (time.perf_counter() - t0)  # ms per 1000 = us per call
        out[name] = {"allowed": len(m), "cold_ms": round(cold, 3), "cached_us": round(cached * 1e3, 2)}
    cur, ids = g.cursor(), []
    t0 = time.perf_counter()
    for _ in range(1000):
        cur(ids)
    out["cursor_call_us"] = round((time.perf_counter() - t0) * 1e3, 2)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["mask", "dense"])
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--V", type=int, default=128256)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--burst", type=int, default=500)
    a = ap.parse_args()
    if a.host:
        return host_cost()
    import torch

    from llm_kubernetes_minikube_sharp4dev_amd import ops

    dev = torch.device("cuda", 0)
    B, V = a.B, a.V
    rng = np.random.default_rng(0)
    sets = [np.sort(rng.choice(V, size=100_000 - 1000 * k, replace=False)) for k in range(8)]
    logits = (torch.randn(B, V, generator=torch.Generator().manual_seed(0)) * 3).to(torch.bfloat16).to(dev)
    upload_ms = None
    if a.arm == "mask":
        words = (V + 31) // 32
        bits = np.zeros((8, words * 32), dtype=np.uint8)
        for k, s in enumerate(sets):
            bits[k, s] = 1
        pool = torch.from_numpy(np.packbits(bits, axis=1, bitorder="little").view(np.int32).copy()).to(dev)
        mrow = torch.arange(B, dtype=torch.int32, device=dev) % 8
        buf = torch.empty(B, V, dtype=torch.float32, device=dev)

        def call():
            return ops.mask_logits(logits, pool, mrow, out=buf)
    else:
        flat = np.concatenate([sets[b % 8] + b * V for b in range(B)])
        ups = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            idx = torch.from_numpy(flat).to(dev, non_blocking=True)
            torch.cuda.synchronize()
            ups.append((time.perf_counter() - t0) * 1e3)
        upload_ms = round(statistics.median(ups), 3)
        sel = torch.arange(B, dtype=torch.int64, device=dev)

        def call():
            mask = torch.full((B, V), float("-inf"), device=dev, dtype=logits.dtype)
            mask.view(-1).index_fill_(0, idx, 0.0)
            logits.index_add_(0, sel, mask)  # idempotent: -inf stays -inf, kept ids get + 0
            return logits.float()

    for _ in range(20):
        call()
    torch.cuda.synchronize()
    per = []
    for _ in range(a.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.burst):
        call()
    e1.record()
    e1.synchronize()
    out = call()
    kept = int((out[:8] != float("-inf")).sum())
    print(json.dumps({"arm": a.arm, "B": B, "V": V, "per_call_us_median": round(statistics.median(per), 2),
                      "per_call_us_min": round(min(per), 2), "burst_us": round(e0.elapsed_time(e1) * 1e3 / a.burst, 2),
                      "ids_upload_ms": upload_ms, "kept_first_8_rows": kept, "want_kept": int(sum(len(s) for s in sets))}))


if __name__ == "__main__":
    main()
