"""A protocol-exact stand-in for an engine core (:mod:`.engine_core`) with no model: every
``gen`` request receives ``tokens`` token ids, one per simulated engine step of ``step_s``
seconds, batched per step and connection exactly like the real core's frames.  For load
tests of the HTTP front-ends / routing (``benchmarks/frontend_load.py``) and CPU tests: it
isolates the serving path's own cost from GPU work."""
from __future__ import annotations

import asyncio
import os
import struct

import msgpack
import numpy as np

_HDR = struct.Struct("<I")


def fake_rerank_logit(query: str, doc: str) -> float:
    """The fake core's score of a pair: a deterministic function of the two texts (CRC-32 of
    ``query NUL doc`` mapped onto [-4, 4)), so front-end tests know every score without a model."""
    import zlib

    return (zlib.crc32((query + "\0" + doc).encode("utf-8")) % 8192) / 1024.0 - 4.0


def fake_rerank_scores(query: str, docs: list, activation: int = 0) -> np.ndarray:
    s = np.array([fake_rerank_logit(query, d) for d in docs], dtype=np.float32)
    return (1.0 / (1.0 + np.exp(-s.astype(np.float64)))).astype(np.float32) if activation else s


class FakeCore:
    def __init__(self, path: str, tokens: int = 48, step_s: float = 0.002, dim: int = 768, vocab: int = 32000):
        self.path, self.tokens, self.step_s, self.dim, self.vocab = path, tokens, step_s, dim, vocab
        self.served = 0
        self.aborted = 0
        self._server = None

    async def start(self):
        if os.path.exists(self.path):
            os.unlink(self.path)
        self._server = await asyncio.start_unix_server(self._conn, path=self.path, limit=1 << 24)

    async def _conn(self, reader, writer):
        active: dict = {}  # rid -> tokens left
        want: dict = {}    # rid -> top_logprobs of a request that asked for logprobs
        lock = asyncio.Lock()

        def send(obj):
            body = msgpack.packb(obj, use_bin_type=True)
            writer.write(_HDR.pack(len(body)) + body)

        async def stepper():
            while True:
                await asyncio.sleep(self.step_s)
                if not active:
                    continue
                items = []
                for rid in list(active):
                    left = active[rid] - 1
                    tid = 1000 + (rid * 7 + left) % 20000
                    if left <= 0:
                        del active[rid]
                        items.append([rid, [tid], True, "length", 0, None])
                        self.served += 1
                    else:
                        active[rid] = left
                        items.append([rid, [tid], False, None, None, None])
                    if rid in want:
                        # the real core's 7th element: one [chosen, [[id, logprob], ...]] per id
                        n = want[rid] if left > 0 else want.pop(rid)
                        items[-1].append([[-0.5, [[tid + j, -0.5 - j] for j in range(n)]]])
                send(["tok", items, [100000, 0, len(active)]])
                await writer.drain()

        task = asyncio.get_running_loop().create_task(stepper())
        try:
            while True:
                n = _HDR.unpack(await reader.readexactly(4))[0]
                msg = msgpack.unpackb(await reader.readexactly(n), raw=False)
                op, rid = msg[0], msg[1]
                if op == "gen":
                    sp = msg[4]
                    active[rid] = min(self.tokens, int(sp.get("max_tokens") or self.tokens))
                    if sp.get("logprobs"):
                        want[rid] = int(sp.get("top_logprobs") or 0)
                elif op == "abort":
                    want.pop(rid, None)
                    if active.pop(rid, None) is not None:
                        self.aborted += 1
                elif op == "load":
                    kind = "rerank" if "rerank" in msg[2] else ("generate" if "embed" not in msg[2] else "embed")
                    send(["load", rid, {"kind": kind, "name": msg[2],
                                        "preset": msg[2], "max_model_len": 8192, "eos_ids": [], "chat_style": "llama3",
                                        "load_s": 0.0, "vocab_size": self.vocab}])
                elif op == "embed":
                    v = np.ones((len(msg[3]), self.dim), np.float32) / np.sqrt(self.dim)
                    send(["emb", rid, v.tobytes(), v.shape[0], v.shape[1]])
                elif op == "rerank":  # (token count: one per whitespace word of each pair)
                    q, docs = msg[3], list(msg[4])
                    s = fake_rerank_scores(q, docs, int(msg[5]) if len(msg) > 5 else 1)
                    ntok = sum(len(q.split()) + len(d.split()) + 3 for d in docs)
                    send(["rr", rid, s.tobytes(), len(docs), ntok])
        except (asyncio.IncompleteReadError, ConnectionError):
            pass
        finally:
            task.cancel()
            writer.close()


async def serve(paths: list[str], tokens: int = 48, step_s: float = 0.002):
    cores = [FakeCore(p, tokens, step_s) for p in paths]
    for c in cores:
        await c.start()
    return cores


def main():  # python -m llm_kubernetes_minikube_sharp4dev_amd.serving.fake_core PATH[,PATH...] [tokens] [step_s]
    import sys

    paths = sys.argv[1].split(",")
    tokens = int(sys.argv[2]) if len(sys.argv) > 2 else 48
    step_s = float(sys.argv[3]) if len(sys.argv) > 3 else 0.002

    async def run():
        await serve(paths, tokens, step_s)
        await asyncio.Event().wait()

    asyncio.run(run())


if __name__ == "__main__":
    main()
