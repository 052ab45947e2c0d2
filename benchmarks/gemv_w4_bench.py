#!/usr/bin/env python3
"""MXFP4 decode GEMV (csrc/gemv_decode_mxfp4.hip) against the bf16 decode GEMV (csrc/gemv_decode.hip) and
the FP8 one (csrc/gemv_decode_w8.hip) in one process: the Llama-3-8B decode projections and the LM
head at M 1 and 2, weights cold (each launch reads the next of enough weight copies that even the
MXFP4 set overflows the 256 MB MALL), back-to-back launches, interleaved rounds; median and
[min, max] of the rounds.  Arms of the MXFP4 kernel: its default plan, pairs per wave 1 / 2 / 4 and
the two-wave K split off / on.  Then the projections of one whole decode step (32 layers of
distinct weights + the LM head, no attention) on the three paths.  Microseconds, TB/s of weight bytes.

    python benchmarks/gemv_w4_bench.py [--m 1,2] [--rounds 5] [--layers 32] [--md out.md]
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
# name: (pairs per wave, K split) of gemv_w4_set_plan; 0 / -1: the kernel's own plan
ARMS = {"mxfp4": (0, -1), "pairs 1": (1, -1), "pairs 2": (2, -1), "pairs 4": (4, -1), "ksplit off": (0, 0),
        "ksplit on": (0, 1)}
BYTES = {"bf16": 2.0, "fp8": 1.0, "mxfp4": 17 / 32}
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
    """The tensors around one projection; ``run(mode, norm, w)`` launches it on bf16 ``w``, on an FP8
    ``(wq, wscale)`` pair or on an MXFP4 ``(wq4, wexp)`` pair (told apart by the second dtype)."""

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
        if not isinstance(w, tuple):
            fn, w, K = self.L.gemv_decode, (w,), w.shape[1]
        elif w[1].dtype == torch.uint8:
            fn, K = self.L.gemv_decode_w4, w[0].shape[1] * 2
        else:
            fn, K = self.L.gemv_decode_w8, w[0].shape[1]
        g = self.g if norm else None
        if mode == 3:
            return fn(3, self.res, *w, g, EPS, None, self.pos, self.cos_sin, Hq, Hkv, D, self.kc, self.vc, self.slots,
                      False)
        if mode == 1:
            return fn(1, self.x[K], *w, None, EPS, self.res)
        return fn(mode, self.res if norm else self.x[K], *w, g, EPS)


QUANT = {"bf16": lambda w: w, "fp8": ops.quantize_rows_e4m3, "mxfp4": ops.quantize_rows_mxfp4}


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
    cols = ["bf16", "fp8", *ARMS]
    lines = ["| M | shape | " + " | ".join(f"{n} us [min, max] (TB/s)" for n in cols) + " |", "|---|---|" + "---|" * len(cols)]
    for M in [int(m) for m in a.m.split(",")]:
        st = Step(M)
        for name in a.shapes.split(","):
            N, K, mode, norm = SHAPES[name]
            n = max(2, -(-600 * 2**20 // int(N * K * BYTES["mxfp4"])))  # copies: the MXFP4 set alone overflows the MALL
            copies = [torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02 for _ in range(n)]
            sets = {k: [q(w) for w in copies] for k, q in QUANT.items()}
            t = {k: [] for k in cols}
            for _ in range(a.rounds):
                for k in ("bf16", "fp8"):
                    t[k].append(timed(lambda w: st.run(mode, norm, w), sets[k]))
                for arm, (pairs, ks) in ARMS.items():
                    L.gemv_w4_set_plan(pairs, ks)
                    t[arm].append(timed(lambda w: st.run(mode, norm, w), sets["mxfp4"]))
                L.gemv_w4_set_plan(0, -1)

            def fmt(k):
                us = statistics.median(t[k])
                return f"{us:.1f} [{min(t[k]):.1f}, {max(t[k]):.1f}] ({N * K * BYTES.get(k, BYTES['mxfp4']) / us / 1e6:.2f})"

            lines.append(f"| {M} | {name} | " + " | ".join(fmt(k) for k in cols) + " |")
            print(lines[-1], flush=True)
            del copies, sets
            torch.cuda.empty_cache()
    if a.layers:
        lines += ["", "| M | whole step: projections of %d layers + LM head | bf16 gemv ms | fp8 ms | mxfp4 ms |" % a.layers,
                  "|---|---|---|---|---|"]
        layers = []
        for _ in range(a.layers):
            ws = {k: torch.randn(SHAPES[k][0], SHAPES[k][1], device=dev, dtype=torch.bfloat16) * 0.02
                  for k in ("qkv", "o", "gate_up", "down")}
            layers.append({kind: {k: q(w) for k, w in ws.items()} for kind, q in QUANT.items()})
        head = torch.randn(*SHAPES["lm_head"][:2], device=dev, dtype=torch.bfloat16) * 0.02
        heads = {kind: q(head) for kind, q in QUANT.items()}
        for M in [int(m) for m in a.m.split(",")]:
            st = Step(M)

            def step(kind):
                for lw in layers:
                    for k in ("qkv", "o", "gate_up", "down"):
                        st.run(SHAPES[k][2], SHAPES[k][3], lw[kind][k])
                st.run(0, False, heads[kind])

            t = {kind: [] for kind in QUANT}
            for _ in range(a.rounds):
                for kind in QUANT:
                    t[kind].append(timed(step, [kind], iters=5) / 1e3)
            lines.append(f"| {M} | | " + " | ".join(f"{statistics.median(t[k]):.3f} [{min(t[k]):.3f}, {max(t[k]):.3f}]"
                                                   for k in QUANT) + " |")
            print(lines[-1], flush=True)
    out = "\n".join(lines)
    print(out)
    if a.md:
        with open(a.md, "w") as f:
            f.write(f"weights cold, median [min, max] of {a.rounds} interleaved rounds x 20 launches\n\n{out}\n")


if __name__ == "__main__":
    main()
