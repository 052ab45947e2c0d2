"""The attention probes through the real ModelRunner on the GPU: which keys a query sees and where
a token's K / V lands, as the runner's metadata, ``paged_attention`` and the split / tile policy of
``ops`` decide them (tests/step_probes.py has the probe model, the table and the driver).

Every case runs probes U, N and W and checks (a) every output row against its float64 answer,
(b) the cache afterwards: the slots of every position run so far hold that token's K / V bit for
bit and every other slot, block 0 included, is still NaN, (c) the rows that feed the LM head.
tests/test_step_probes_cpu.py shows what these comparisons reject."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_probes as P  # noqa: E402
import step_probes as SP  # noqa: E402
from step_probes import same_bits  # noqa: E402

from llm_kubernetes_minikube_sharp4dev_amd import ops  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.engine import model_runner  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.models import attention  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ["U", "N", "W"]
SHAPES = [(4, 128), (1, 64)]
SPLITS = {1: 128, 3: 128, 16: 256, 64: 512, 256: 2048}


def _steps(drv, steps, what):
    for i, items in enumerate(steps):
        drv.run(items, f"{what}, step {i}", cache=False)
    drv.check_cache(what)


class World:
    """One scene over the contexts of attn_probes.DECODE_CTX for the cases that decode: the float64
    answers of the prefill that writes them are computed once per (probe, G, D) and shared; each
    driver (eager, graphed) writes its own cache through its own runner."""

    def __init__(self, kind, G, D):
        sc = self.scene = SP.Scene(kind, G, D)
        self.w, self.setup = SP.plan_contexts(sc, P.DECODE_CTX)
        self.decode = SP.plan_decode(sc, P.DECODE_CTX, w=self.w)[1]
        self.graph = SP.plan_graph_decode(sc, w=self.w)[1]
        self.mixed_setup, self.mixed = SP.plan_mixed(sc, w=self.w)
        self.inflight = SP.plan_inflight(sc, w=self.w)[1]
        self.drivers = {}

    def driver(self, graphs):
        if graphs not in self.drivers:
            drv = SP.Driver(self.scene, DEV, use_graphs=graphs)
            _steps(drv, self.setup, "prefill of the contexts")
            self.drivers[graphs] = drv
        return self.drivers[graphs]


@functools.lru_cache(maxsize=None)
def world(kind, G=4, D=128):
    return World(kind, G, D)


# ---- prefill -------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,D", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_chunked_and_batched_prefill(kind, G, D):
    """A 300-token sequence as chunks (100, 7, 193) whose starts are neither block- nor tile-aligned,
    each step shared with the whole prefill of two or three other sequences, then the (chunk, past)
    pairs of attn_probes.PREFILL_QP: ``prefill_tiles`` orders tiles across sequences."""
    sc = SP.Scene(kind, G, D)
    steps = SP.plan_prefill(sc)
    drv = SP.Driver(sc, DEV)
    mixed_order = 0
    for i, items in enumerate(steps):
        res = drv.run(items, f"chunked prefill {kind} G{G} D{D}, step {i}")
        assert res.si.num_decode == 0 and len(res.si.q_lens) == len(items)
        ts, _ = ops.prefill_tiles(res.si.q_lens, res.si.ctx_lens, G, True, D)
        mixed_order += bool((np.diff(ts) < 0).any())
    assert mixed_order >= 3, "the tile order never left the sequence order"


@pytest.mark.parametrize("kind", KINDS)
def test_prefix_hit(kind):
    """B's block table names the first 4 blocks A's prefill wrote; B prefills from position 64."""
    sc = SP.Scene(kind)
    steps = SP.plan_prefix_hit(sc)
    drv = SP.Driver(sc, DEV)
    drv.run(steps[0], f"prefix hit {kind}, A")
    res = drv.run(steps[1], f"prefix hit {kind}, B from 64")
    assert res.seqs[0].block_table[:4] == drv.blocks[steps[0][0].seq.kg][:4]
    assert res.si.ctx_lens == [150] and res.si.q_lens == [86]


# ---- mixed steps ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_mixed_step_overlap_variants(kind, monkeypatch):
    """Prefill chunks and decode rows in one step: the paged decode on the side stream, the flash
    prefill on the side stream, and no overlap give the answer and the same bits."""
    wd = world(kind)
    drv = wd.driver(False)
    _steps(drv, wd.mixed_setup, f"mixed {kind}, setup")
    got = {}
    for name, on, side in (("decode on the side", True, "decode"), ("flash on the side", True, "flash"),
                           ("no overlap", False, "decode")):
        monkeypatch.setattr(attention, "OVERLAP_ATTN", on)
        monkeypatch.setattr(attention, "ATTN_SIDE", side)
        res = drv.run(wd.mixed, f"mixed {kind}, {name}")
        assert res.si.num_decode == 5 and res.si.q_lens == [70, 50] and res.si.ctx_lens == [70, 90]
        got[name] = res.kept
    for name in got:
        assert same_bits(got[name], got["no overlap"]), f"mixed {kind}: {name} differs from no overlap"


# ---- eager decode --------------------------------------------------------------------------------
def _eager_decode(kind, G, D):
    wd = world(kind, G, D)
    drv = wd.driver(False)
    r = drv.runner
    for B in SP.BATCHES + (3,):  # and a smaller batch after the largest
        assert r.decode_split(B)[0] == SPLITS[B]
        for b, items in enumerate(wd.decode[B]):
            what = f"decode {kind} G{G} D{D} B {B} batch {b}"
            res = drv.run(items, what, cache=False)
            assert res.si.num_decode == B and not res.si.q_lens and not res.si.decode_graph
            # again: the tickets and _decode_ws as the first run left them
            again = drv.run(items, what + " again", cache=False)
            assert same_bits(res.kept, again.kept), f"{what}: the second run differs"
        drv.check_cache(f"decode {kind} G{G} D{D} B {B}")
        if B * SP.HKV >= 512:
            t = ops.decode_tickets(r.device, B * SP.HKV)
            assert int(t[: B * SP.HKV].abs().sum()) == 0, "a ticket was not reset"


@pytest.mark.parametrize("kind", KINDS)
def test_eager_decode_every_split_policy(kind):
    """B = 1, 3, 16, 64, 256 rows: B * Hkv = 2, 6, 32, 128, 512 and splits 128, 128, 256, 512 and
    2048 with the fused-merge tickets; rows repeat the contexts of attn_probes.DECODE_CTX (sharing
    their blocks), which sit on both sides of every split edge; each batch twice in a row."""
    _eager_decode(kind, 4, 128)


@pytest.mark.parametrize("kind", KINDS)
def test_eager_decode_small_heads(kind):
    _eager_decode(kind, 1, 64)


# ---- hipGraph decode -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_graph_decode_replays(kind):
    """B = 3 in bucket 4 and B = 5 in bucket 8, with padding rows: each captured bucket replayed with
    three different sets of sequences, contexts and block tables; the larger bucket is captured after
    the smaller (``_decode_ws`` regrows), then the smaller one is replayed again.  Bit-identical to
    the eager runner on the same inputs."""
    wd = world(kind)
    eager = wd.driver(False)
    graphed = SP.Driver(wd.scene, DEV, use_graphs=True)  # its own: no bucket captured yet
    _steps(graphed, wd.setup, f"graph decode {kind}, setup")
    r = graphed.runner
    ws = []
    for B, bucket, batches in ((3, 4, wd.graph[3]), (5, 8, wd.graph[5]), (3, 4, wd.graph[3][:1])):
        assert r.decode_split(B)[0] == r.decode_split(bucket)[0] == 128
        for b, items in enumerate(batches):
            what = f"graph decode {kind} B {B} replay {b}"
            res = graphed.run(items, what)
            assert res.si.decode_graph == bucket and res.si.num_decode == B
            ref = eager.run(items, what + " (eager)")
            assert same_bits(res.kept, ref.kept), f"{what}: graph and eager differ"
        ws.append(r._ws[0].numel())
    assert ws[0] < ws[1] == ws[2] and set(r.graphs) == {(4, False), (8, False)}


# ---- extend chunks -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_extend_chunks_as_decode_rows(kind, monkeypatch):
    """Items (seq, start, n) of n = 2, 5 and 16 generated tokens: causal decode rows, eager and graphed
    (where the sampled row is a subset gathered after the replay), and with EXTEND_AS_DECODE = 0 a
    flash-prefill chunk.  All n rows of each route against the answer."""
    sc = SP.Scene(kind)
    setup, items = SP.plan_extend(sc)
    drivers = {name: SP.Driver(sc, DEV, use_graphs=name == "graphed") for name in ("eager", "graphed", "flash")}
    kept = {}
    for name, drv in drivers.items():
        monkeypatch.setattr(model_runner, "EXTEND_AS_DECODE", 0 if name == "flash" else 16)
        _steps(drv, setup, f"extend {kind}, setup")
        for its in [[it] for it in items] + [items]:
            T = sum(it.n for it in its)
            what = f"extend {kind} {[(it.start, it.n) for it in its]}, {name}"
            res = drv.run(its, what)
            assert len(res.index) == T and len(res.si.logits_rows) == len(its)
            assert res.si.num_decode == (0 if name == "flash" else T)
            if name == "graphed":
                bucket = drv.runner._graph_bucket(T)
                assert res.si.decode_graph == bucket and len(res.si.logits_rows) != res.si.num_decode
                assert drv.runner.decode_split(T)[0] == drv.runner.decode_split(bucket)[0]
            kept[name, T] = res.kept
    for T in (2, 5, 16, 23):
        assert same_bits(kept["eager", T], kept["graphed", T]), f"extend {kind}, {T} rows: graph and eager differ"


# ---- cascade -------------------------------------------------------------------------------------
def _cascade(kind, monkeypatch):
    monkeypatch.setenv("LK_CASCADE", "1")
    sc = SP.Scene(kind)
    setup, plan = SP.plan_cascade(sc)
    drivers = {"eager": SP.Driver(sc, DEV), "graphed": SP.Driver(sc, DEV, use_graphs=True)}
    for drv in drivers.values():
        assert drv.runner.cascade
        _steps(drv, setup, f"cascade {kind}, setup")
    return plan, drivers


@pytest.mark.parametrize("kind", KINDS)
def test_cascade_decode(kind, monkeypatch):
    """Batches whose rows share 0, 1, 3 and 18 leading blocks (one shared block gives shared_len 0;
    the first row's context is shared + 1) and one whose shortest row clamps the run below the
    blocks in common; eager and graphed.  The batches alternate, so the one captured graph is
    replayed with shared_len 0 and > 0 in turn."""
    plan, drivers = _cascade(kind, monkeypatch)
    order = ["0 shared blocks", "3 shared blocks", "1 shared blocks", "18 shared blocks", "clamped"]
    assert sorted(order) == sorted(plan)
    seen = []
    for t in range(max(len(b) for _, b in plan.values())):
        for label in order:
            shared, batches = plan[label]
            if t >= len(batches):
                continue
            for name, drv in drivers.items():
                res = drv.run(batches[t], f"cascade {kind}, {label}, copy {t}, {name}", cache=t == 0)
                assert res.si.shared_len == shared, f"{label}: shared_len {res.si.shared_len}, want {shared}"
                assert res.si.decode_graph == (8 if name == "graphed" else 0) and res.si.num_decode == 5
            seen.append(shared)
    assert seen[:5] == [0, 48, 0, 288, 32]
    assert set(drivers["graphed"].runner.graphs) == {(8, False)}
    for drv in drivers.values():
        drv.check_cache(f"cascade {kind}")


# ---- in-flight ids -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_inflight_ids_from_prev_ids(kind):
    """Decode rows whose id the host does not have yet (it passes 0, another probe row): the id comes
    from ``runner.prev_ids`` at ``inflight_row``, in another order than this step's rows."""
    wd = world(kind)
    kept = {}
    for graphs in (False, True):
        drv = wd.driver(graphs)
        res = drv.run(wd.inflight, f"in-flight ids {kind}, {'graphed' if graphs else 'eager'}")
        assert res.host_ids[:5].tolist() == [0] * 5 and res.si.gather[1].tolist() == list(SP.INFLIGHT_ROWS)
        assert res.si.decode_graph == (8 if graphs else 0)
        kept[graphs] = res.kept
    assert same_bits(kept[False], kept[True]), f"in-flight ids {kind}: graph and eager differ"


# ---- what the GPU-only logic's probes reject -----------------------------------------------------
def _rejected(run):
    try:
        run()
    except AssertionError as e:
        return str(e)
    return None


def test_probes_reject_a_shared_len_one_block_long(monkeypatch):
    """``_shared_len`` one block too long: every row then takes keys 48 .. 63 from the first row's
    block, which stays inside valid, written blocks.  U and W cannot see it (their K and V depend on
    the position alone); N does: its V rows differ per sequence."""
    out = {}
    for kind in KINDS:
        monkeypatch.setenv("LK_CASCADE", "1")
        sc = SP.Scene(kind)
        setup, plan = SP.plan_cascade(sc, (3,))
        drv = SP.Driver(sc, DEV)
        _steps(drv, setup, "setup")
        orig = drv.runner._shared_len
        drv.runner._shared_len = lambda bt, ctx, n: orig(bt, ctx, n) + SP.BS

        def run():
            for t, items in enumerate(plan["3 shared blocks"][1]):
                rows = items[2:]  # contexts past the longer prefix: every row keeps a key of its own
                assert all(it.start + 1 > 64 for it in rows)
                res = drv.step(rows)
                assert res.si.shared_len == 64
                drv.check_rows(res, f"shared_len one block long, {kind}, copy {t}")
        out[kind] = _rejected(run)
        print(f"{kind}: {out[kind]}")
    assert out["N"] is not None and "probe N" in out["N"] and out["U"] is None and out["W"] is None


def test_probes_reject_a_chunk_that_loses_a_tile(monkeypatch):
    """The tile list of a chunk with a past built one tile early: every q0 is still a tile start of
    its sequence (so the launch stays inside its tables), the chunk's first tile runs twice and its
    last not at all.  (``past`` itself only enters the cost that orders the tiles, which no output
    depends on.)  Every probe rejects the rows left unwritten."""
    orig = ops.prefill_tiles

    def early(q_lens, ctx_lens, G, causal, D=128):
        ts, tq = orig(q_lens, ctx_lens, G, causal, D)
        qb = ops.prefill_rows_per_tile(G, D)
        past = np.asarray(ctx_lens)[ts] - np.asarray(q_lens)[ts]
        return ts, np.where(past > 0, np.maximum(tq - qb, 0), tq).astype(np.int32)

    for kind in KINDS:
        sc = SP.Scene(kind)
        steps = SP.plan_prefill(sc)
        drv = SP.Driver(sc, DEV)
        drv.run(steps[0], "first chunk")
        drv.run(steps[1], "second chunk")
        monkeypatch.setattr(ops, "prefill_tiles", early)
        msg = _rejected(lambda: drv.run(steps[2], f"a chunk that loses its last tile, {kind}"))
        monkeypatch.setattr(ops, "prefill_tiles", orig)
        print(f"{kind}: {msg}")
        assert msg is not None and "non-finite" in msg
