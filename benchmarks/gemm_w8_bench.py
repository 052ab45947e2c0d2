#!/usr/bin/env python3
"""FP8 decode GEMM for 3 to 16 rows (csrc/gemm_decode_w8.hip) against what the same step runs on the
bf16 weights (ops.linear_rope_kv, ops.linear_add_rmsnorm, ops.linear_swiglu, ops.linear: the
weight-streaming GEMMs with their split-K consumers) in one process: the Llama-3-8B decode
projections and the LM head at M 4, 8 and 16, weights cold (each launch reads the next of enough
weight copies that even the FP8 set overflows the 256 MB MALL), back-to-back launches, interleaved
rounds; median and [min, max] of the rounds.  Arms of the FP8 kernel: its default plan, 4 / 8 waves
per workgroup, the K split over 1 / 2 / 4 / 8 waves, 1 / 2 units per wave.  ``route`` is the rule of
ops.gemm_w8_supported: yes where the default plan's median beats the bf16 median by more than the
two arms' [min, max] spreads together.  Then the projections of one whole decode step (32 layers of
distinct weights + the LM head, no attention) on both routes.  Microseconds, TB/s of weight bytes.

    python benchmarks/gemm_w8_bench.py [--m 4,8,16] [--rounds 5] [--layers 32] [--md out.md]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from llm_kubernetes_minikube_sharp4dev_amd import ops  # noqa: E402

# name: (N, K, mode of the FP8 kernel, norm prologue)
SHAPES = {"qkv": (6144, 4096, 3, True), "o": (4096, 4096, 1, False), "gate_up": (28672, 4096, 2, True),
          "down": (4096, 14336, 1, False), "lm_head": (128256, 4096, 0, False)}
# name: (waves per workgroup, K-split waves, units per wave) of gemm_w8_set_plan; 0: the kernel's own plan
ARMS = {"fp8": (0, 0, 0), "w4": (4, 0, 0), "w8": (8, 0, 0), "kw1": (0, 1, 0), "kw2": (0, 2, 0), "kw4": (0, 4, 0),
        "w8kw8": (8, 8, 0), "P1": (0, 0, 1), "P2": (0, 1, 2)}
BYTES = {"bf16": 2.0, "fp8": 1.0}
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
    """The tensors around one projection; ``run(name, w)`` launches it on bf16 ``w`` (the route of a
    step without the option) or on an FP8 ``(wq, wscale)`` pair."""

    def __init__(self, M, dev="cuda"):
        self.L = ops.lib()  # (the binding itself: the wrapper's argument checks are host time)
        self.cos_sin = ops.rope_cos_sin(8192, D, 500000.0, None, device=dev)
        self.pos = torch.full((M,), 700, dtype=torch.int32, device=dev)
        self.slots = torch.arange(M, dtype=torch.int32, device=dev) + 5 * BS
        self.kc = torch.zeros(64, Hkv, BS, D, device=dev, dtype=torch.bfloat16)
        self.vc = torch.zeros_like(self.kc)
        self.x = {K: torch.randn(M, K, device=dev, dtype=torch.bfloat16) for K in (4096, 14336)}
        self.res = torch.randn(M, 4096, device=dev, dtype=torch.bfloat16)
        self.g = torch.ones(4096, device=dev, dtype=torch.bfloat16)

    def run(self, name, w):
        _, K, mode, norm = SHAPES[name]
        if isinstance(w, tuple):
            g = self.g if norm else None
            if mode == 3:
                return self.L.gemm_decode_w8(3, self.res, *w, g, EPS, None, self.pos, self.cos_sin, Hq, Hkv, D, self.kc,
                                             self.vc, self.slots, False)
            if mode == 1:
                return self.L.gemm_decode_w8(1, self.x[K], *w, None, EPS, self.res)
            return self.L.gemm_decode_w8(mode, self.res if norm else self.x[K], *w, g, EPS)
        if name == "qkv":  # (its input was normed by the projection before it)
            return ops.linear_rope_kv(self.x[K], w, self.pos, self.cos_sin, Hq, Hkv, D, self.kc, self.vc, self.slots,
                                      False, False)
        if mode == 1:  # residual add and the next norm ride on the split-K consumer
            return ops.linear_add_rmsnorm(self.x[K], w, self.res, self.g, EPS)
        return ops.linear_swiglu(self.x[K], w) if mode == 2 else ops.linear(self.x[K], w)


def fmt(ts, nbytes):
    us = statistics.median(ts)
    return f"{us:.1f} [{min(ts):.1f}, {max(ts):.1f}] ({nbytes / us / 1e6:.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", default="4,8,16")
    ap.add_argument("--shapes", default="qkv,o,gate_up,down,lm_head")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32, help="layers of the whole-step run (0: skip it)")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    dev = "cuda"
    Ms = [int(m) for m in a.m.split(",")]
    cols = ["bf16", *ARMS]
    lines = ["| M | shape | " + " | ".join(f"{n} us [min, max] (TB/s)" for n in cols) + " | route |",
             "|---|---|" + "---|" * (len(cols) + 1)]
    for name in a.shapes.split(","):
        N, K, _, _ = SHAPES[name]
        n = max(2, -(-600 * 2**20 // int(N * K * BYTES["fp8"])))  # copies: the FP8 set alone overflows the MALL
        copies = [torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02 for _ in range(n)]
        quant = [ops.quantize_rows_e4m3(w) for w in copies]
        for M in Ms:
            st = Step(M)
            t = {k: [] for k in cols}
            for _ in range(a.rounds):
                t["bf16"].append(timed(lambda w: st.run(name, w), copies))
                for arm, plan in ARMS.items():
                    ops.gemm_w8_set_plan(*plan)
                    t[arm].append(timed(lambda w: st.run(name, w), quant))
                ops.gemm_w8_set_plan(0, 0, 0)
            gain = statistics.median(t["bf16"]) - statistics.median(t["fp8"])
            spread = max(t["bf16"]) - min(t["bf16"]) + max(t["fp8"]) - min(t["fp8"])
            lines.append(f"| {M} | {name} | " + " | ".join(fmt(t[k], N * K * BYTES.get(k, BYTES["fp8"])) for k in cols)
                         + f" | {'yes' if gain > spread else 'no'} |")
            print(lines[-1], flush=True)
        del copies, quant
        torch.cuda.empty_cache()
    if a.layers:
        lines += ["", "| M | whole step: projections of %d layers + LM head | bf16 route ms | fp8 ms |" % a.layers,
                  "|---|---|---|---|"]
        layers = []
        for _ in range(a.layers):
            ws = {k: torch.randn(SHAPES[k][0], SHAPES[k][1], device=dev, dtype=torch.bfloat16) * 0.02
                  for k in ("qkv", "o", "gate_up", "down")}
            layers.append({"bf16": ws, "fp8": {k: ops.quantize_rows_e4m3(w) for k, w in ws.items()}})
        head = torch.randn(*SHAPES["lm_head"][:2], device=dev, dtype=torch.bfloat16) * 0.02
        heads = {"bf16": head, "fp8": ops.quantize_rows_e4m3(head)}
        for M in Ms:
            st = Step(M)

            def step(kind):
                for lw in layers:
                    for k in ("qkv", "o", "gate_up", "down"):
                        st.run(k, lw[kind][k])
                st.run("lm_head", heads[kind])

            t = {"bf16": [], "fp8": []}
            for _ in range(a.rounds):
                for kind in t:
                    t[kind].append(timed(step, [kind], iters=5) / 1e3)
            lines.append(f"| {M} | | " + " | ".join(f"{statistics.median(v):.3f} [{min(v):.3f}, {max(v):.3f}]"
                                                   for v in t.values()) + " |")
            print(lines[-1], flush=True)
    out = "\n".join(lines)
    print(out)
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write(f"weights cold, median [min, max] of {a.rounds} interleaved rounds x 20 launches\n\n{out}\n")


if __name__ == "__main__":
    main()
