"""The attention probes of tests/attn_probes.py run through the real serving loop: ``LLMEngine``
(``_launch`` / ``_sample`` / ``_collect``, ``step()`` and ``step_pipelined()``, ``_jump``), the
``Scheduler`` (admission, chunking, ``_preempt``, ``_admit_prefix``, ``publish_blocks``), the block
allocator (Python and native) and the ``ModelRunner`` fed by real previous steps.

tests/step_probes.py builds every step by hand.  Here nothing above the model is built by hand: a
scenario adds requests and calls ``step()`` / ``step_pipelined()`` until the engine is idle, and what
the scheduler ran, whatever it was, is checked afterwards.

The scripted model.  ``ScriptedModel`` is ``step_probes.ProbeModel`` (embed, ``kv_write``, NaN-filled
output, ``paged_attention``, the kept rows) whose "LM head" answers ``id + 1``: the ids of a writer
sequence of a ``Scene`` are consecutive, so the token after the row with input id ``t`` is ``t + 1``.
``greedy`` returns those ids, ``logits`` an f32 one-hot at them; both are torch ops of static shape
and capture into a hipGraph.

Rows identify themselves.  A token id names one (writer sequence, position).  After every
``runner.execute`` the step's device ids, positions, slots and kept attention rows are cloned on the
runner's stream (the static buffers of the bucket after a graph replay, the last forward's after an
eager step) and read on the host when the scenario is over, so a pipelined run stays pipelined.  Every
logged row with a non-zero id must carry the position its id names and the float64 attention answer
of that (sequence, position), under the derived tolerances of probes U and N (two bf16 half-ulps,
one bf16 ulp; W is left out: its tolerance is measured over fixed shapes, and here the shapes are the
scheduler's).  The rows left out are graph padding (id 0, slot -1), and the number of rows checked
in a step must equal the number of tokens the scheduler put into it.  The tokens of every request
must be its script, bit for bit, and after every collect the slots of positions [0, num_computed)
of every running sequence, found through its own block table, must hold its K and V bit for bit; so
must all 16 slots of a block at the collect that publishes it to the prefix cache.

A scenario may not pass without having met the situation it names (``Spec.post``).

The schedule depends on the host loop alone and the tokens are scripted, so the CPU run (reference
ops) and the GPU run (HIP kernels, graphs or not, either probe, either head size, either allocator)
of a scenario see the same schedule: ``STEPS`` records the launches of the CPU run
(tests/test_engine_probes_cpu.py asserts them) and tests/test_engine_exact_gpu.py asserts its own
count against it.

Per scenario, synchronous / pipelined (CPU run; the same for U and N; rows = attention rows
checked; hits = tokens served by the prefix cache at admission; evictions = hashed blocks the
allocator took back; F is the small scenario of the scheduler fix, CPU only):

  scenario      steps      rows         preemptions  hits       evictions
  A             214 / 214  880 / 880    0 / 0        0 / 0      0 / 0
  A64 (D 64)    214 / 214  880 / 880    0 / 0        0 / 0      0 / 0
  B             373 / 375  760 / 760    0 / 0        400 / 400  24 / 26
  C             219 / 219  700 / 721    3 / 5        80 / 176   27 / 26
  C-nocache     219 / 229  2389 / 2570  40 / 39      0 / 0      0 / 0
  D             129 / 158  880 / 880    0 / 0        0 / 0      0 / 0
  D-tight       132 / 161  703 / 690    4 / 3        128 / 96   25 / 25
  E             214 / 214  880 / 880    0 / 0        0 / 0      0 / 0
  F             42 / 42    132 / 132    0 / 0        16 / 16    2 / 2

On an MI355X with graphs the steps split into replays + eager steps (synchronous / pipelined): A and
A64 193 + 21 / 193 + 21, B 359 + 14 / 361 + 14, C 202 + 17 / 201 + 18, C-nocache 126 + 93 / 129 + 100,
D 106 + 23 / 135 + 23, D-tight 114 + 18 / 144 + 17, E 193 + 21 / 193 + 21; of the pipelined steps, 213 of
A's 214 and 139 of D's 158 gather in-flight ids on the device.
GPU wall time as measured there, per test of tests/test_engine_exact_gpu.py (scene, engine, every
step, the checks): 0.08 - 0.28 s, and 0.87 s for the first, which loads the library; the 64 tests
together 10.7 s.

Plain torch, importable on the CPU; the tests import this module as a sibling."""
import os
import sys
from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_probes as SP  # noqa: E402

from llm_kubernetes_minikube_sharp4dev_amd import ops  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.engine.block_manager import BlockAllocator  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.engine.llm_engine import LLMEngine  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.engine.model_runner import ModelRunner  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.engine.sampling import SamplingParams  # noqa: E402

BS = SP.BS
MAX_MODEL_LEN = 1024
MAX_NUM_SEQS = 8
LIMIT = 3000  # iterations of the host loop after which a scenario counts as stuck

# launches of each scenario's CPU run, (synchronous, pipelined): the GPU runs must take as many
STEPS = {
    "A": (214, 214), "A64": (214, 214), "B": (373, 375), "C": (219, 219), "C-nocache": (219, 229),
    "D": (129, 158), "D-tight": (132, 161), "E": (214, 214), "F": (42, 42),
}


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
class ScriptedModel(SP.ProbeModel):
    """ProbeModel's attention; the next token of the row with input id t is t + 1."""

    def __init__(self, scene, device):
        super().__init__(scene, device)
        # table rows + 2, rounded up to whole 32-byte rows of f32 logits, which ops.select_tokens asks for
        self.cfg = SimpleNamespace(num_layers=1, vocab_size=-(-(self.table.shape[0] + 2) // 8) * 8, eos_token_ids=())
        self.last = None  # (ids, positions, slots) of the last forward Python ran

    def __call__(self, ids, meta, kv_caches):
        super().__call__(ids, meta, kv_caches)
        self.last = (ids, meta.positions, meta.slots)
        rows = ids if meta.logits_idx is None else ops.gather_rows(ids, meta.logits_idx)
        return rows + 1

    def greedy(self, h):
        return h

    def logits(self, h, gather=True, dtype=None):
        out = torch.zeros((h.shape[0], self.cfg.vocab_size), dtype=torch.float32, device=h.device)
        return out.scatter_(1, h.long().unsqueeze(1), 1.0)


# ------------------------------------------------------------------------------------------------
# scenarios
# ------------------------------------------------------------------------------------------------
@dataclass
class Req:
    """One request: the first ``plen`` ids of ``seq`` as the prompt, the rest as the expected tokens.
    mode: "plain" (plain greedy: the ids come from the model), "logprobs" (greedy through the
    sampler), "forced" (a logits_processor that forces output k when k % 7 in (2, 3, 4))."""
    name: str
    seq: object
    plen: int
    mode: str = "plain"


@dataclass
class Spec:
    name: str
    scene: object
    script: list            # [(when(harness) -> bool, [Req])]: phases, started in order
    num_blocks: int = 128
    budget: int = 24
    prefix: bool = True
    post: object = None     # post(harness): the conditions of the scenario
    expect_cached: dict = field(default_factory=dict)  # request -> num_cached_prefix


def every(k, n=3):
    return lambda h: h.it >= n * k


def done(*names):
    return lambda h: all(h.reqs[n].finished for n in names)


def needles(n):
    return SP.prefill_needles(n)


def writer(sc, name, n):
    return sc.seq(name, sc.keys(n), needles=needles(n))


def sharer(sc, name, n, base, shared):
    return sc.seq(name, sc.keys(n, base=base.kg, shared=shared), q_from=shared, needles=needles(n))


GEOM_A = ((5, 40), (33, 140), (70, 130), (100, 300), (200, 270))   # ample pool
GEOM_C = ((5, 40), (33, 140), (70, 130), (100, 200), (17, 60))     # 38 blocks through a pool of 14
TIGHT = 14


def _staggered(sc, geom, modes):
    script = []
    for k, ((plen, n), mode) in enumerate(zip(geom, modes)):
        script.append((every(k), [Req(f"r{k}", writer(sc, f"s{plen}-{n}", n), plen, mode)]))
    return script


def spec_A(kind, D=128, modes=("plain",) * 5, name="A"):
    """Continuous batching: staggered arrivals, a 24-token budget (prompt chunks share steps with
    decode rows and end off the block grid), requests that finish at different steps."""
    sc = SP.Scene(kind, 4, D)

    def post(h):
        s = h.stats
        assert s["mixed"] > 0, "A: no step mixed prompt chunks and decode rows"
        assert s["off_grid_chunks"] > 0, "A: no chunk boundary off the block grid"
        assert s["preemptions"] == 0
        if len(set(modes)) > 1:
            assert s["greedy_steps"] > 0 and s["sampled_steps"] > 0, "E: one route only"
    return Spec(name, sc, _staggered(sc, GEOM_A, modes), post=post)


def spec_E(kind):
    """A again, every other request greedy through the sampler (logprobs): steps alternate between
    the ids-from-model and the sampler route."""
    return spec_A(kind, modes=("plain", "logprobs", "plain", "logprobs", "plain"), name="E")


def spec_B(kind):
    """Prefix cache, pool of 20 blocks, budget 40."""
    sc = SP.Scene(kind)
    W = writer(sc, "W", 170)
    S1 = sharer(sc, "S1", 100, W, 64)
    S2 = sharer(sc, "S2", 160, W, 128)
    S3 = sharer(sc, "S3", 80, W, 64)
    S4 = sharer(sc, "S4", 100, W, 64)
    X1 = writer(sc, "X1", 310)  # 20 blocks: the whole pool
    X0 = writer(sc, "X0", 40)   # 3 more, so that the pool's order is not the one it started with
    script = [
        (every(0), [Req("W", W, 140)]),                                   # (i)
        (done("W"), [Req("S1", S1, 80), Req("S2", S2, 135)]),             # (ii) hits on freed blocks
        (done("S1", "S2"), [Req("S3", S3, 70)]),                          # (iii) the first holder
        (lambda h: len(h.reqs["S3"].output_ids) >= 2, [Req("S4", S4, 66)]),   # ... a hit on its live blocks
        (done("S3", "S4"), [Req("X1", X1, 100)]),                         # (iv) evicts everything
        (done("X1"), [Req("X0", X0, 5)]),
        (done("X0"), [Req("S1b", S1, 80)]),                               # (v) the sharer again: a miss
        (done("S1b"), [Req("T", S1, 96)]),                                # (vi) 6 full blocks, all cached
    ]

    def post(h):
        assert h.admit_refs["S4"] == [2] * 4, f"B (iii): reference counts {h.admit_refs['S4']} of the shared blocks"
        assert h.admit_refs["S1"] == [1] * 4 and h.admit_refs["S2"] == [2] * 4 + [1] * 4
        assert h.reqs["S3"].step_finish < h.reqs["S4"].step_finish, "B (iii): the first holder did not finish first"
        assert h.stats["evictions"] > 0, "B: no hashed block was evicted"
        assert h.stats["preemptions"] == 0
        old, new = h.tables["S1"][:4], h.tables["S1b"][:4]
        assert old != new, f"B (v): the prefix was recomputed into the same blocks {old}"
    return Spec("B", sc, script, num_blocks=20, budget=40, post=post,
                expect_cached={"W": 0, "S1": 64, "S2": 128, "S3": 64, "S4": 64, "X1": 0, "X0": 0, "S1b": 0, "T": 80})


def spec_C(kind, prefix=True, modes=("plain",) * 5, name=None, budget=24):
    """Preemption: five requests of 38 blocks through a pool of 14."""
    sc = SP.Scene(kind)
    name = name or ("C" if prefix else "C-nocache")

    def post(h):
        s = h.stats
        assert s["preemptions"] > 1, f"{name}: {s['preemptions']} preemptions"
        assert sum(r.num_preemptions for r in h.reqs.values()) == s["preemptions"]
        if h.pipelined:
            assert s["preempted_inflight"] > 0, f"{name}: no victim had a token in flight"
        if prefix:
            assert s["readmit_hits"] > 0, f"{name}: no re-admission was served from the prefix cache"
        else:
            assert s["hits"] == 0, f"{name}: a prefix hit without a prefix cache"
        if "forced" in modes:
            _post_jump(h, name)
    return Spec(name, sc, _staggered(sc, GEOM_C, modes), num_blocks=TIGHT, budget=budget, prefix=prefix, post=post)


def _post_jump(h, name):
    s = h.stats
    assert s["jumped"] > 0, f"{name}: nothing jumped"
    assert s["extend_as_decode"] > 0, f"{name}: no extend chunk ran as decode rows"
    if h.pipelined:  # (synchronously the token before a jump is never in flight)
        assert s["discards"] > 0, f"{name}: discard_rows was never used"


def spec_D(kind, tight=False):
    """Jump-forward through the real _jump: every request forces outputs k % 7 in (2, 3, 4)."""
    if tight:
        return spec_C(kind, modes=("forced",) * 5, name="D-tight")
    sc = SP.Scene(kind)
    return Spec("D", sc, _staggered(sc, GEOM_A, ("forced",) * 5), post=lambda h: _post_jump(h, "D"))


def spec_F(kind):
    """The smallest scenario in which a waiting sequence's prefix-cache hit starved a preempted one:
    pool of 5 blocks.  P leaves two hashed blocks behind; A (33 -> 60, 4 blocks) decodes; Q, a sharer
    of P's two blocks, arrives when only they are left, so its admission takes them and then fails;
    A outgrows its 3 blocks, is its own victim and goes in front of Q.  With Q holding the two blocks
    and nothing running, A (4 blocks) did not fit the 3 that were left and was finished as an error.
    Now Q gives the hit back when its admission fails, and A takes the two cached blocks instead of
    being preempted (tests/test_engine_probes_cpu.py runs it with a waiting sequence that keeps them)."""
    sc = SP.Scene(kind)
    P = writer(sc, "P", 40)
    A = writer(sc, "A", 60)
    Q = sharer(sc, "Q", 48, P, 32)
    script = [(every(0), [Req("P", P, 36)]), (done("P"), [Req("A", A, 33)]),
              (lambda h: len(h.reqs["A"].output_ids) >= 2, [Req("Q", Q, 40)])]

    def post(h):
        assert h.stats["dropped_hits"] > 0, "F: no waiting sequence gave a prefix hit back"
    return Spec("F", sc, script, num_blocks=5, budget=64, post=post)


SPECS = {
    "A": spec_A, "A64": lambda kind: spec_A(kind, 64, name="A64"), "B": spec_B, "C": spec_C,
    "C-nocache": lambda kind: spec_C(kind, prefix=False), "D": spec_D,
    "D-tight": lambda kind: spec_D(kind, tight=True), "E": spec_E, "F": spec_F,
}


# ------------------------------------------------------------------------------------------------
# the harness
# ------------------------------------------------------------------------------------------------
def _lookup(scene):
    """Per id: (index of the sequence that owns it, position); the float64 answers, by id."""
    if getattr(scene, "_by_id", None) is None:
        n = scene.table().shape[0]
        owner = np.full(n, -1, dtype=np.int64)
        pos = np.full(n, -1, dtype=np.int64)
        ans = torch.zeros(n, scene.Hq, scene.D, dtype=torch.float64)
        for i, s in enumerate(scene.seqs):
            own = np.asarray(s.ids[s.q_from:], dtype=np.int64)
            assert (np.diff(own) == 1).all() and (owner[own] == -1).all()
            owner[own], pos[own] = i, np.arange(s.q_from, s.n)
            ans[own[0]: own[-1] + 1] = scene.want(s, s.q_from, s.n)  # once per sequence
        assert (owner[1:] >= 0).all()
        scene._by_id = (owner, pos, ans)
    return scene._by_id


def script_of(req):
    s = req.seq
    return list(s.ids[req.plen:s.n]) + [s.ids[s.n - 1] + 1]


class Harness:
    def __init__(self, spec, device="cpu", graphs=False, pipelined=False, allocator=None, mutate=None):
        self.spec, self.scene, self.pipelined = spec, spec.scene, pipelined
        self.device = torch.device(device)
        self.model = ScriptedModel(spec.scene, device)
        r = self.runner = ModelRunner(self.model, BS, MAX_MODEL_LEN, MAX_NUM_SEQS, spec.num_blocks, use_graphs=graphs)
        assert r.num_blocks == spec.num_blocks
        r.kv.fill_(float("nan"))
        e = self.eng = LLMEngine(self.model, None, BS, MAX_MODEL_LEN, MAX_NUM_SEQS, spec.budget, spec.prefix, graphs,
                                 spec.num_blocks, eos_ids=set(), _runner=r)
        if allocator == "python":
            e.allocator = e.scheduler.alloc = BlockAllocator(spec.num_blocks, BS, spec.prefix)
        elif allocator == "native":
            from llm_kubernetes_minikube_sharp4dev_amd.native import runtime
            e.allocator = e.scheduler.alloc = runtime.NativeBlockAllocator(spec.num_blocks, BS, spec.prefix)
        self.reqs, self.req_of, self.tables, self.admit_refs = {}, {}, {}, {}
        self.log, self.cache_log, self._published = [], [], []
        self.it = self.phase = 0
        self.stats = dict.fromkeys(("preemptions", "preempted_inflight", "readmit_hits", "evictions", "jumped",
                                    "discards", "extend_as_decode", "mixed", "off_grid_chunks", "replays", "eager",
                                    "gathers", "greedy_steps", "sampled_steps", "hits", "rows", "dropped_hits"), 0)
        mutate and mutate(self)
        self._hooks()

    # ---- the hooks: records around the engine's own methods, which stay as they are
    def _hooks(self):
        e, r, sch, al, st = self.eng, self.runner, self.eng.scheduler, self.eng.allocator, self.stats
        fwd, exe, collect, jump = r.forward_logits, r.execute, e._collect, e._jump
        preempt, admit, alloc, register = sch._preempt, sch._admit_prefix, al.allocate, al.register
        drop, publish = sch._drop_prefix, sch.publish_blocks
        hashed = {}  # block -> hash, as register() published it: the blocks an allocate() can evict
        known = set()
        info = {}

        def forward_logits(items, greedy=False):
            info.clear()
            info.update(ntok=sum(n for _, _, n in items), greedy=greedy)
            for seq, start, n in items:
                ext = start >= len(seq.prompt_ids) and n > 1
                st["extend_as_decode"] += bool(ext and r._as_decode(seq, start, n))
                st["off_grid_chunks"] += bool(start < len(seq.prompt_ids) and (start + n) % BS
                                              and start + n < len(seq.prompt_ids))
            st["greedy_steps" if greedy else "sampled_steps"] += 1
            return fwd(items, greedy)

        def execute(si):
            out = exe(si)
            if si.decode_graph:  # the replay wrote the bucket's static buffers; Python ran no forward
                g = r.graphs[(si.decode_graph, si.greedy)]
                ids, pos, slots, keep = g["ids"], g["pos"], g["slots"], self.model._keep[si.decode_graph]
                st["replays"] += 1
            else:
                (ids, pos, slots), keep = self.model.last, self.model.kept
                st["eager"] += 1
            st["mixed"] += bool(si.q_lens and si.num_decode)
            st["gathers"] += si.gather is not None
            self.log.append((len(self.log), si.decode_graph, info["ntok"], ids.clone(), pos.clone(), slots.clone(),
                             keep.clone()))
            return out

        def _collect(pending):
            out = collect(pending)
            self._queue_cache_check()
            return out

        def _jump(seq, now):
            before = seq.discard_rows
            jump(seq, now)
            st["discards"] += seq.discard_rows - before

        def _preempt(seq):
            st["preemptions"] += 1
            st["preempted_inflight"] += seq.num_inflight == 1
            preempt(seq)

        def _admit_prefix(seq):
            fresh = seq.num_computed == 0 and not seq.block_table
            admit(seq)
            if fresh:
                name = self.req_of[seq.req_id]
                st["hits"] += seq.num_computed
                st["readmit_hits"] += bool(seq.num_preemptions and seq.num_computed)
                if not seq.num_preemptions:
                    self.admit_refs[name] = [al.ref[b] for b in seq.block_table]

        def publish_blocks(seq):  # the blocks it registers go into the next cache check
            before = seq.num_hashed_blocks
            publish(seq)
            for j in range(before, seq.num_hashed_blocks):
                self._published.append((seq.user["name"], j, seq.block_table[j],
                                        seq.user["pseq"].ids[j * BS:(j + 1) * BS]))

        def _drop_prefix(seq):  # the admission failed: the hit just counted served nothing
            if seq.block_table:
                st["dropped_hits"] += 1
                st["hits"] -= seq.num_computed
                st["readmit_hits"] -= bool(seq.num_preemptions)
            drop(seq)

        def allocate():
            b = alloc()
            h = hashed.pop(b, None)
            if h is not None:  # a block that still answered to a hash: evicted; the hash can be published again
                st["evictions"] += 1
                known.discard(h)
            return b

        def reg(block, parent, tokens):
            h = register(block, parent, tokens)
            if self.spec.prefix and h not in known:
                known.add(h)
                hashed[block] = h
            return h

        r.forward_logits, r.execute, e._collect, e._jump = forward_logits, execute, _collect, _jump
        sch._preempt, sch._admit_prefix, al.allocate, al.register = _preempt, _admit_prefix, allocate, reg
        sch._drop_prefix, sch.publish_blocks = _drop_prefix, publish_blocks

    # ---- requests
    def add(self, rq):
        s = rq.seq
        assert s.q_from < rq.plen < s.n, "generation must start inside the sequence's own ids"
        want = script_of(rq)
        if rq.mode == "plain":
            p = SamplingParams.greedy(len(want))
        elif rq.mode == "logprobs":
            p = SamplingParams.greedy(len(want), logprobs=True)
        else:
            def proc(out, want=want):
                k = len(out)
                return [want[k]] if k % 7 in (2, 3, 4) else None
            p = SamplingParams.greedy(len(want), logits_processor=proc)
        seq = self.eng.add_request(list(s.ids[:rq.plen]), p)
        seq.user.update(name=rq.name, pseq=s, want=want)
        self.reqs[rq.name] = seq
        self.req_of[seq.req_id] = rq.name
        return seq

    # ---- the cache check, queued on the runner's stream
    def _to_dev(self, a):
        t = torch.from_numpy(np.ascontiguousarray(a))
        if self.device.type == "cuda":
            return t.pin_memory().to(self.device, non_blocking=True)
        return t

    def _queue_cache_check(self):
        slots, ids, who = [], [], []
        for seq in self.eng.scheduler.running:
            n = min(seq.num_computed, seq.user["pseq"].n)
            if not n:
                continue
            p = np.arange(n, dtype=np.int64)
            bt = np.asarray(seq.block_table, dtype=np.int64)
            assert len(bt) * BS >= n, f"cache: {seq.user['name']} has {len(bt)} blocks for {n} computed tokens"
            slots.append(bt[p // BS] * BS + p % BS)
            ids.append(np.asarray(seq.user["pseq"].ids[:n], dtype=np.int64))
            who.append((seq.user["name"], n, list(seq.block_table)))
            self.tables[seq.user["name"]] = list(seq.block_table)
        for name, j, blk, toks in self._published:  # a published block holds all 16 tokens it was hashed over
            assert len(toks) == BS, f"cache: block {j} of {name} was published over {len(toks)} tokens"
            slots.append(blk * BS + np.arange(BS, dtype=np.int64))
            ids.append(np.asarray(toks, dtype=np.int64))
            who.append((f"{name} as published (its block {j})", BS, [blk]))
        self._published = []
        if not slots:
            return
        slots, ids = self._to_dev(np.concatenate(slots)), self._to_dev(np.concatenate(ids))
        hq, hkv, D = self.model.hq, self.model.hkv, self.model.D
        kc, vc = self.runner.kv_caches[0]
        blk, off = slots // BS, slots % BS
        want = self.model.table.index_select(0, ids)[:, hq * D:].view(torch.int16)
        got = torch.cat([kc[blk, :, off].reshape(-1, hkv * D), vc[blk, :, off].reshape(-1, hkv * D)], dim=1)
        bad = (got.view(torch.int16) != want).any(dim=1)
        self.cache_log.append((self.eng.steps, who, bad))

    # ---- the host loop
    def run(self):
        e, script = self.eng, self.spec.script
        while True:
            while self.phase < len(script) and script[self.phase][0](self):
                for rq in script[self.phase][1]:
                    self.add(rq)
                self.phase += 1
            if self.phase == len(script) and not e.has_work() and not e.in_flight:
                break
            try:
                if not self.pipelined:
                    e.step()
                elif e.has_work():
                    e.step_pipelined()
                else:
                    e.flush()
            except IndexError as err:  # (the reference ops; the HIP embedding counts such ids: embed_errors)
                raise AssertionError(f"rows: iteration {self.it} indexed outside the table or the step: {err}") from None
            self.it += 1
            assert self.it < LIMIT, "tokens: the scenario does not finish: " + ", ".join(
                f"{n} has {len(s.output_ids)} of {len(s.user['want'])}" for n, s in self.reqs.items() if not s.finished)
        e.flush()
        return self.finish()

    # ---- the checks
    def finish(self):
        sc, kind, st = self.scene, self.scene.kind, self.stats
        what = f"{self.spec.name} {kind} {'pipelined' if self.pipelined else 'synchronous'}"
        for name, seq in self.reqs.items():
            want = seq.user["want"]
            if seq.output_ids != want:
                k = next((i for i, (a, b) in enumerate(zip(seq.output_ids, want)) if a != b),
                         min(len(want), len(seq.output_ids)))
                raise AssertionError(f"{what}: tokens of {name}: {len(seq.output_ids)} of {len(want)}, first "
                                     f"difference at output {k}: got {seq.output_ids[k:k + 3]}, want {want[k:k + 3]}")
            assert seq.finish_reason == "length", f"{what}: tokens of {name}: finish reason {seq.finish_reason}"
        # the rows
        owner, posn, ans = _lookup(sc)
        seen = np.zeros(len(owner), dtype=bool)
        for k, graph, ntok, ids, pos, slots, keep in self.log:
            ids, pos, slots = ids.cpu().numpy().astype(np.int64), pos.cpu().numpy(), slots.cpu().numpy()
            w = f"{what}, step {k}" + (f" (graph {graph})" if graph else "")
            nz = ids != 0
            assert ((slots >= 0) == nz).all() and (graph or nz.all()), f"{w}: rows with id 0 that are no padding"
            assert int(nz.sum()) == ntok, f"{w}: rows: {int(nz.sum())} carry an id, {ntok} tokens were scheduled"
            assert ids.max() < len(owner), f"{w}: rows: id {ids.max()} is outside the scene"
            rid = ids[nz]
            if (pos[nz] != posn[rid]).any():
                j = int(np.nonzero(pos[nz] != posn[rid])[0][0])
                raise AssertionError(f"{w}: row {j} has the id of ({sc.seqs[owner[rid[j]]].name}, {posn[rid[j]]}) "
                                     f"at position {pos[nz][j]}")
            got = keep.cpu().view(len(ids), sc.Hq, sc.D)[torch.from_numpy(nz)]
            want = ans[torch.from_numpy(rid)]
            try:
                SP.check(kind, got, want, w)
            except AssertionError as e:
                x = torch.nan_to_num(SP.excess(kind, got, want), nan=float("inf")).flatten(1).amax(dim=1)
                bad = torch.nonzero(x > 1).flatten().tolist()
                raise AssertionError(f"{e} -- rows are (sequence, position): " + ", ".join(
                    f"row {j} = ({sc.seqs[owner[rid[j]]].name}, {posn[rid[j]]})" for j in bad[:6])) from None
            seen[rid] = True
            st["rows"] += len(rid)
        missing = np.nonzero(~seen[1:])[0] + 1
        if len(missing):
            raise AssertionError(f"{what}: rows: {len(missing)} (sequence, position) pairs never ran, first "
                                 f"({sc.seqs[owner[missing[0]]].name}, {posn[missing[0]]})")
        # the cache
        if self.cache_log:
            bad = torch.cat([b for _, _, b in self.cache_log]).cpu()
            if bool(bad.any()):
                i = int(torch.nonzero(bad)[0])
                for step, who, b in self.cache_log:
                    if i < len(b):
                        for name, n, table in who:
                            if i < n:
                                raise AssertionError(f"{what}: cache after collect {step}: position {i} of {name} "
                                                     f"(block {table[i // BS]}, offset {i % BS}) does not hold its K / V")
                            i -= n
                    i -= len(b)
        al = self.eng.allocator
        assert al.num_free == self.spec.num_blocks, f"{what}: cache: {al.num_free} of {self.spec.num_blocks} blocks free"
        assert all(al.ref[b] == 0 for b in range(self.spec.num_blocks)), f"{what}: cache: a reference count is left"
        for name, n in self.spec.expect_cached.items():
            got = self.reqs[name].num_cached_prefix
            assert got == n, f"{what}: {name} was served {got} tokens from the prefix cache, expected {n}"
        st["jumped"] = sum(s.jumped for s in self.reqs.values())
        st["steps"] = self.eng.launches
        assert len(self.log) == self.eng.launches
        if self.spec.post:
            self.spec.post(self)
        return st
