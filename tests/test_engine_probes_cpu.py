"""What the engine probes of tests/engine_probes.py accept and reject, on the CPU (where ops fall back
to ops/reference.py): every scenario passes through the real LLMEngine, Scheduler and allocator,
synchronous and pipelined, with probes U and N, having met the situation it names; scenarios B and C
pass with the Python and the native allocator; and each listed mutation of the scheduler, the
allocator, the runner or the engine makes its scenario fail with a row, token or cache message.
tests/test_engine_exact_gpu.py runs the same scenarios over the HIP kernels."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_probes as EP  # noqa: E402

from llm_kubernetes_minikube_sharp4dev_amd.engine.block_manager import BlockAllocator, make_allocator  # noqa: E402

MODES = [False, True]
MODE_IDS = ["step", "pipelined"]


def run(name, kind, pipelined, allocator=None, mutate=None):
    h = EP.Harness(EP.SPECS[name](kind), pipelined=pipelined, allocator=allocator, mutate=mutate)
    return h, h.run()


@pytest.mark.parametrize("pipelined", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("kind", ["U", "N"])
@pytest.mark.parametrize("name", list(EP.SPECS))
def test_scenario_passes(name, kind, pipelined):
    h, st = run(name, kind, pipelined)
    print(f"\n{name} {kind} {MODE_IDS[pipelined]}: {({k: v for k, v in st.items() if v})}")
    assert st["rows"] >= h.scene.table().shape[0] - 1 and st["replays"] == 0
    assert st["gathers"] > 0 if pipelined else st["gathers"] == 0
    if name in EP.STEPS:  # the count the GPU runs are held to
        assert st["steps"] == EP.STEPS[name][pipelined]


def _allocators():
    native = type(make_allocator(4, 16)) is not BlockAllocator
    return ["python", "native"] if native else ["python"]


@pytest.mark.parametrize("pipelined", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("allocator", _allocators())
@pytest.mark.parametrize("name", ["B", "C", "F"])
def test_either_allocator(name, allocator, pipelined):
    h, st = run(name, "N", pipelined, allocator)
    assert (type(h.eng.allocator) is BlockAllocator) == (allocator == "python")
    assert h.eng.scheduler.alloc is h.eng.allocator
    assert st["steps"] == EP.STEPS[name][pipelined]


# ---- the mutations -------------------------------------------------------------------------------
def m_allocate_live_block(h):
    """Every fifth allocate() hands out the last block of a running sequence (and counts the new
    reference, so the books still balance at the end)."""
    a, n = h.eng.allocator, [0]
    orig = a.allocate

    def allocate():
        n[0] += 1
        held = [s for s in h.eng.scheduler.running if s.block_table]
        if n[0] % 5 == 0 and held:
            b = held[0].block_table[-1]
            a.ref[b] += 1
            return b
        return orig()
    a.allocate = allocate


def m_match_prefix_shifted(h):
    a = h.eng.allocator
    orig = a.match_prefix

    def match_prefix(tokens):
        blocks, parent = orig(tokens)
        return blocks[1:] + blocks[:1], parent  # the same blocks (and references), one place on
    a.match_prefix = match_prefix


def m_preempt_keeps_num_computed(h):
    sch = h.eng.scheduler
    orig = sch._preempt

    def _preempt(seq):
        n = seq.num_computed
        orig(seq)
        seq.num_computed = n
    sch._preempt = _preempt


def m_publish_up_to_length(h):
    sch = h.eng.scheduler

    def publish_blocks(seq):
        full = seq.length // sch.bs
        while seq.num_hashed_blocks < full and seq.num_hashed_blocks < len(seq.block_table):
            j = seq.num_hashed_blocks
            toks = seq.tokens(j * sch.bs, (j + 1) * sch.bs)
            seq.last_hash = sch.alloc.register(seq.block_table[j], seq.last_hash, toks)
            seq.num_hashed_blocks += 1
    sch.publish_blocks = publish_blocks


def m_gather_next_row(h):
    r = h.runner
    orig = r._gather

    def _gather(dec, offset):
        g = orig(dec, offset)
        if g is None:
            return g
        return g[0], (g[1] + 1) % r.prev_ids.shape[0]  # (the last row takes the first: still a row of prev_ids)
    r._gather = _gather


def m_collect_keeps_discard_rows(h):
    e = h.eng
    orig = e._collect

    def _collect(pending):
        before = {id(s): s.discard_rows for s, _ in pending[1] or []}
        out = orig(pending)
        for s, _ in pending[1] or []:
            if before[id(s)]:
                s.discard_rows = before[id(s)]
        return out
    e._collect = _collect


def m_waiting_keeps_its_hit(h):
    """The scheduler as it was: a waiting sequence whose admission failed kept its prefix-cache hit."""
    h.eng.scheduler._drop_prefix = lambda seq: None


# mutation -> (how, scenario, allocator, the modes it must fail in)
MUTATIONS = {
    "allocate hands out a block that is still referenced": (m_allocate_live_block, "C", "python", MODES),
    "match_prefix returns its hit shifted by one block": (m_match_prefix_shifted, "B", "python", MODES),
    "_preempt keeps num_computed": (m_preempt_keeps_num_computed, "C-nocache", None, MODES),
    "publish_blocks registers up to length // bs": (m_publish_up_to_length, "C", None, MODES),
    "_gather takes inflight_row + 1": (m_gather_next_row, "A", None, [True]),
    "_collect skips the discard_rows decrement": (m_collect_keeps_discard_rows, "D", None, [True]),
    "a waiting sequence keeps its prefix hit": (m_waiting_keeps_its_hit, "F", None, MODES),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_mutation_is_rejected(name):
    mutate, scenario, allocator, modes = MUTATIONS[name]
    print()
    for kind in "UN":
        for pipelined in modes:
            try:
                run(scenario, kind, pipelined, allocator, mutate)
                msg = None
            except AssertionError as e:
                msg = str(e)
            print(f"{name} / {scenario} {kind} {MODE_IDS[pipelined]}: {('passes' if msg is None else msg)[:300]}")
            assert msg is not None, f"'{name}' passes scenario {scenario} ({kind}, {MODE_IDS[pipelined]})"
            assert any(w in msg for w in ("row", "tokens", "cache")), msg
