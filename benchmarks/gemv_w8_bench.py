#!/usr/bin/env python3
"""FP8 decode GEMV (csrc/gemv_decode_w8.hip) against the bf16 decode GEMV (csrc/gemv_decode.hip) in one
process: the Llama-3-8B decode projections and the LM head at M 1 and 2, weights cold (each launch
reads the next of enough weight copies to overflow the 256 MB MALL), back-to-back launches, medians
of interleaved rounds; then the projections of one whole decode step (32 layers of distinct weights
+ the LM head, no attention) on both paths.  Arms of the FP8 kernel: its default plan, the other
pairs-per-wave setting, and the two-wave K split off.  Prints microseconds and TB/s of weight bytes.

    python benchmarks/gemv_w8_bench.py [--m 1,2] [--rounds 5] [--layers 32] [--md out.md]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from llm_kubernetes_minikube_sharp4dev_amd import ops  # noqa: E402

# name: (N, K, gemv mode, norm prologue)
SHAPES = {"qkv": (6144, 4096, 3, True), "o": (4096, 4096, 1, False), "gate_up": (28672, 4096, 2, True),
          "down": (4096, 14336, 1, False), "lm_head": (128256, 4096, 0, False)}
# name: (pairs per wave, K split) of gemv_w8_set_plan; 0 / -1: the kernel's own plan
ARMS = {"fp8": (0, -1), "fp8 pairs 1": (1, -1), "fp8 pairs 2": (2, -1), "fp8 ksplit off": (0, 0), "fp8 ksplit on": (0, 1)}
Hq, Hkv, D, BS, EPS = 32, 8, 128, 16, 1e-5


def timed(fn, copies, iters=20):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn(copies[0])
    torch.cuda.synchronize()
    ev[0].record()
    for i in range(iters):
        fn(copies[i % len(copies)])
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / iters


class Step:
    """The tensors around one projection; ``run(mode, norm, w)`` launches it on bf16 ``w`` or on an
    FP8 ``(wq, wscale)`` pair."""

    def __init__(self, M, dev="cuda"):
        self.L = ops.lib()
        self.cos_sin = ops.rope_cos_sin(8192, D, 500000.0, None, device=dev)
        self.pos = torch.full((M,), 700, dtype=torch.int32, device=dev)
        self.slots = torch.arange(M, dtype=torch.int32, device=dev) + 5 * BS
        self.kc = torch.zeros(64, Hkv, BS, D, device=dev, dtype=torch.bfloat16)
        self.vc = torch.zeros_like(self.kc)
        self.x = {K: torch.randn(M, K, device=dev, dtype=torch.bfloat16) for K in (4096, 14336)}
        self.res = torch.randn(M, 4096, device=dev, dtype=torch.bfloat16)
        self.g = torch.ones(4096, device=dev, dtype=torch.bfloat16)

    def run(self, mode, norm, w):
        fp8 = isinstance(w, tuple)
        fn = self.L.gemv_decode_w8 if fp8 else self.L.gemv_decode
        w = w if fp8 else (w,)
        K = w[0].shape[1]
        g = self.g if norm else None
        if mode == 3:
            return fn(3, self.res, *w, g, EPS, None, self.pos, self.cos_sin, Hq, Hkv, D, self.kc, self.vc, self.slots,
                      False)
        if mode == 1:
            return fn(1, self.x[K], *w, None, EPS, self.res)
        return fn(mode, self.res if norm else self.x[K], *w, g, EPS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", default="1,2")
    ap.add_argument("--shapes", default="qkv,o,gate_up,down,lm_head")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32, help="layers of the whole-step run (0: skip it)")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    dev = "cuda"
    L = ops.lib()
    lines = ["| M | shape | bf16 MB | bf16 gemv us (TB/s) | " + " | ".join(f"{n} us (TB/s)" for n in ARMS) + " |",
             "|---|---|---|---|" + "---|" * len(ARMS)]
    for M in [int(m) for m in a.m.split(",")]:
        st = Step(M)
        for name in a.shapes.split(","):
            N, K, mode, norm = SHAPES[name]
            n = max(2, -(-600 * 2**20 // (N * K)))  # copies: the FP8 set alone overflows the MALL
            copies = [torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02 for _ in range(n)]
            qcopies = [ops.quantize_rows_e4m3(w) for w in copies]
            t = {k: [] for k in ("bf16", *ARMS)}
            for _ in range(a.rounds):
                t["bf16"].append(timed(lambda w: st.run(mode, norm, w), copies))
                for arm, (pairs, ks) in ARMS.items():
                    L.gemv_w8_set_plan(pairs, ks)
                    t[arm].append(timed(lambda w: st.run(mode, norm, w), qcopies))
            L.gemv_w8_set_plan(0, -1)

            def fmt(ts, nbytes):
                us = statistics.median(ts)
                return f"{us:.1f} ({nbytes / us / 1e6:.2f})"

            lines.append(f"| {M} | {name} | {N * K * 2 / 2**20:.0f} | {fmt(t['bf16'], N * K * 2)} | "
                         + " | ".join(fmt(t[arm], N * K) for arm in ARMS) + " |")
            print(lines[-1], flush=True)
            del copies, qcopies
            torch.cuda.empty_cache()
    if a.layers:
        lines += ["", "| M | whole step: projections of %d layers + LM head | bf16 gemv ms | fp8 ms |" % a.layers, "|---|---|---|---|"]
        layers = []
        for _ in range(a.layers):
            ws = {k: torch.randn(SHAPES[k][0], SHAPES[k][1], device=dev, dtype=torch.bfloat16) * 0.02
                  for k in ("qkv", "o", "gate_up", "down")}
            layers.append((ws, {k: ops.quantize_rows_e4m3(w) for k, w in ws.items()}))
        head = torch.randn(*SHAPES["lm_head"][:2], device=dev, dtype=torch.bfloat16) * 0.02
        heads = (head, ops.quantize_rows_e4m3(head))
        for M in [int(m) for m in a.m.split(",")]:
            st = Step(M)

            def step(which):
                for lw in layers:
                    for k in ("qkv", "o", "gate_up", "down"):
                        st.run(SHAPES[k][2], SHAPES[k][3], lw[which][k])
                st.run(0, False, heads[which])

            t = {0: [], 1: []}
            for _ in range(a.rounds):
                for which in (0, 1):
                    t[which].append(timed(step, [which], iters=5) / 1e3)
            lines.append(f"| {M} | | {statistics.median(t[0]):.3f} | {statistics.median(t[1]):.3f} |")
            print(lines[-1], flush=True)
    out = "\n".join(lines)
    print(out)
    if a.md:
        with open(a.md, "w") as f:
            f.write(f"weights cold, median of {a.rounds} interleaved rounds x 20 launches\n\n{out}\n")


if __name__ == "__main__":
    main()
