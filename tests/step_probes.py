"""The probes of tests/attn_probes.py run through the real ModelRunner: a weightless probe model, a
table whose token ids carry the probes' Q / K / V, and a driver that steps real Sequence objects.

tests/test_attention_exact_gpu.py calls the attention bindings with hand-built block tables, context
lengths and tiles over a cache it fills itself.  Here those come from the layer above: the runner's
``_prepare`` / ``_prepare_graph`` / ``_decode_rows`` / ``_slots`` / ``_shared_len`` / ``_meta`` /
``_cascade_meta`` / ``_static`` / ``_graph_execute`` / ``_decode_ws``, ``paged_attention`` with its
side-stream overlap, and the split / merge-route / tile-order policy of ``ops``.  The only K / V a
step can read is what earlier steps wrote through the runner's slots: the cache starts as NaN.

A token id names one (sequence, position) pair.  Row ``id`` of the table is [Q | K | V]: the query
that sequence asks at that position and the key / value of its key group at that position.  Several
sequences may read one key group (decode rows that repeat a context, as ``attn_probes.build_N``
repeats them, share its cache blocks), and a key group may start with the blocks of another (a
prefix-cache hit, a cascade prefix); K depends on (position, kv head) alone in every probe, V on the
position alone in U and W, and N's random V is copied over the shared positions.

The float64 answer of a row is ``attn_probes.exact_attention`` over the keys at positions <= its
own.  Plain torch, importable on the CPU; the tests import this module as a sibling."""
import bisect
import math
import os
import sys
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_probes as P  # noqa: E402

from llm_kubernetes_minikube_sharp4dev_amd import ops  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.engine.model_runner import ModelRunner  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.engine.sampling import SamplingParams  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.engine.sequence import Sequence  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.models.attention import paged_attention  # noqa: E402

BF = torch.bfloat16
HKV, BS = 2, 16
MAX_MODEL_LEN = 4608  # block tables 288 wide: a one-row batch launches 36 splits of 128

# W through the runner: twice the worst relative error of attn_probes.emulate() against the float64
# answer over w_shapes(), the (context, split, k_start) and (chunk, past) shapes of
# tests/test_step_attention_gpu.py -- the splits 256 and 512 included, which RTOL_W was not measured
# over.  The factor 2 is attn_probes': exp2f and the accumulation order are not modelled.  Measured by
# measure_rtol_w_step() (tests/test_step_probes_cpu.py asserts the constant is 2 x what it measures,
# rounded up in the third digit): 0.7074 % (the prefill chunk of positions 0 .. 126, D 128).  The new
# splits do not raise it: it is the value RTOL_W rests on, found at a prefill row there as well.
RTOL_W_STEP = 2 * 0.00708


# ------------------------------------------------------------------------------------------------
# the scene: key groups, sequences, the table
# ------------------------------------------------------------------------------------------------
@dataclass(eq=False)
class PSeq:
    """One sequence of a scene: token ids for positions [0, n), queries for [q_from, n)."""
    name: str
    kg: int
    n: int
    q_from: int
    ids: list
    q: torch.Tensor  # [n - q_from, Hq, D] bf16


@dataclass
class It:
    """One item of a step: tokens [start, start + n) of ``seq``.  mode: "prefill" (a chunk of a
    prompt of ``plen`` tokens, default: the chunk ends it), "decode" (the sequence's one generated
    token), "extend" (generated tokens the host appended: a jump-forward chunk), "inflight" (a
    decode row whose id sits in row ``row`` of the previous step's device ids)."""
    seq: PSeq
    start: int
    n: int
    mode: str = "prefill"
    plen: Optional[int] = None
    row: int = -1


class Scene:
    def __init__(self, kind, G=4, D=128, seed=3):
        assert kind in "UNW"
        self.kind, self.G, self.D, self.Hq = kind, G, D, HKV * G
        self.scale = 1 / math.sqrt(D)
        self.gen = torch.Generator().manual_seed(seed)
        self.K, self.V, self.base, self.shared = [], [], [], []
        self.seqs, self.writer = [], {}
        # id 0 is what the host passes for an id it does not have: a row of its own, unlike any probe's
        w = (self.Hq + 2 * HKV) * D
        decoy = torch.zeros(1, w)
        decoy[:, self.Hq * D: (self.Hq + HKV) * D] = 0.5
        decoy[:, (self.Hq + HKV) * D:] = -3.0
        self._rows = [P._bf16_exact(decoy)[0]]
        self._next = 1
        self._want = {}
        self._table = None

    # ---- keys
    def keys(self, n, base=None, shared=0):
        """A key group of n positions; its first ``shared`` (a multiple of the block size) are those
        of group ``base``, whose cache blocks it then names instead of blocks of its own."""
        assert 0 < n < (1 << P.NEEDLE_BITS) and shared % BS == 0 and shared <= n
        D = self.D
        j = torch.arange(n)
        if self.kind == "N":
            k = torch.stack([P._code(j, D, h) for h in range(HKV)], dim=1)
            v = torch.randint(1, 256, (n, HKV, D), generator=self.gen) / 64.0
            v = v * (2.0 * torch.randint(0, 2, (n, HKV, D), generator=self.gen) - 1.0)
        else:
            k = torch.zeros(n, HKV, D)
            if self.kind == "W":
                wb = torch.tensor(P.W_BASE)
                for h in range(HKV):
                    k[:, h, 0] = wb[(j // 32 + h) % 5] + ((37 * j) % 29) / 32.0
            v = P._onehot_v(n, HKV, D)
        k, v = P._bf16_exact(k, v)
        if shared:
            assert shared <= self.K[base].shape[0]
            v[:shared] = self.V[base][:shared]
            assert torch.equal(k[:shared], self.K[base][:shared])
        self.K.append(k), self.V.append(v), self.base.append(base), self.shared.append(shared)
        return len(self.K) - 1

    # ---- queries
    def _q(self, n, q_from, needles, rot):
        R, G, D = n - q_from, self.G, self.D
        q = torch.zeros(R, self.Hq, D)
        if self.kind == "U":
            q[:] = 1.0
        elif self.kind == "W":
            q[:, :, 0] = 8.0
        else:
            # the needle: c times the binary code of the key asked for, in the rotation of
            # attn_probes.build_N -- a prefill row walks the listed positions it sees plus its own,
            # copy ``rot`` of a decode row the listed positions G at a time
            c = 16.0 * math.floor(20.0 / self.scale / 16.0)
            L = sorted(needles)
            want = torch.zeros(R, HKV, G, dtype=torch.long)
            for r in range(R):
                i = q_from + r
                cand = L[: bisect.bisect_right(L, i)]
                if rot is None:
                    cand = cand + [i]
                for h in range(HKV):
                    for g in range(G):
                        want[r, h, g] = cand[((i if rot is None else rot * G) + g + 3 * h) % len(cand)]
            for h in range(HKV):
                q[:, h * G:(h + 1) * G] = c * P._code(want[:, h].reshape(-1), D, h).view(R, G, D)
        return P._bf16_exact(q)[0]

    def seq(self, name, kg, n=None, q_from=0, needles=(0,), rot=None):
        """A sequence over key group ``kg``.  ``q_from`` > 0: it only ever runs positions from there
        on (a decode copy of a context another sequence prefilled, whose ids it carries below)."""
        n = self.K[kg].shape[0] if n is None else n
        assert self._table is None and 0 <= q_from < n <= self.K[kg].shape[0]
        if q_from:
            ids = self._lower_ids(kg, q_from)
        else:
            ids = []
        new = n - q_from
        ids = ids + list(range(self._next, self._next + new))
        self._next += new
        q = self._q(n, q_from, needles, rot)
        k, v = self.K[kg][q_from:n], self.V[kg][q_from:n]
        self._rows.append(torch.cat([q.reshape(new, -1), k.reshape(new, -1), v.reshape(new, -1)], dim=1))
        s = PSeq(name, kg, n, q_from, ids, q)
        self.seqs.append(s)
        self.writer.setdefault(kg, s)
        return s

    def _lower_ids(self, kg, upto):
        """Ids of positions [0, upto) as the sequences that wrote them carried them (never read by a
        step that starts above them; a real engine's sequence would hold them all the same)."""
        w = self.writer.get(kg)
        if w is not None:
            got = list(w.ids[:upto])
        elif self.base[kg] is not None:
            got = self._lower_ids(self.base[kg], min(upto, self.shared[kg]))
        else:
            got = []
        return got + [0] * (upto - len(got))

    def table(self):
        if self._table is None:
            self._table = torch.cat(self._rows).contiguous()
            assert self._table.dtype == BF and self._table.shape[0] == self._next
        return self._table

    # ---- answers
    def want(self, s, a, b):
        """float64 answers of positions [a, b) of sequence s: [b - a, Hq, D]."""
        key = (id(s), a, b)
        if key not in self._want:
            assert s.q_from <= a < b <= s.n
            K, V = self.K[s.kg], self.V[s.kg]
            q = s.q[a - s.q_from: b - s.q_from]
            G = self.G
            # U and W ask the same of every head of a group: answer one head per group
            qg = q.view(-1, HKV, G, self.D)
            same = G > 1 and bool((qg == qg[:, :, :1]).all())
            if same:
                q = qg[:, :, 0]
            out = []
            for c0 in range(a, b, 256):
                c1 = min(c0 + 256, b)
                mask = torch.arange(c1)[None, :] <= torch.arange(c0, c1)[:, None]
                out.append(P.exact_attention(q[c0 - a: c1 - a], K[:c1], V[:c1], mask, self.scale)[0])
            o = torch.cat(out)
            self._want[key] = o.repeat_interleave(G, dim=1) if same else o
        return self._want[key]


def tolerance(kind, want):
    if kind == "W":
        return RTOL_W_STEP * want.double().abs() + P.FLOOR
    return P.tolerance(kind, want)


def excess(kind, got, want):
    """attn_probes.excess under tolerance() above."""
    d = (got.double() - want.double()).abs()
    t = tolerance(kind, want)
    inf = torch.full_like(d, float("inf"))
    return torch.where(t > 0, d / t.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), inf))


def check(kind, got, want, what=""):
    """attn_probes.check; W the same comparison against RTOL_W_STEP, measured over the shapes run here."""
    if kind != "W":
        return P.check(kind, got, want, what)
    assert torch.isfinite(got.double()).all(), f"{what}: non-finite output"
    x = excess(kind, got, want)
    if bool((x > 1).any()):
        i = int(x.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), x.shape))
        raise AssertionError(f"{what}: probe {kind}: {int((x > 1).sum())} of {x.numel()} elements off; worst at "
                             f"{idx}: got {float(got.double().flatten()[i])!r}, want "
                             f"{float(want.double().flatten()[i])!r} ({float(x.flatten()[i]):.3g} x tolerance)")


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
class ProbeModel:
    """One "layer" without weights: the calls a decoder makes between its QKV GEMM and its output
    projection.  No gemm_shapes / decode_gemm_shapes: the runner tunes nothing.  Every op is a HIP
    launcher or a fill / copy, so the forward captures into a hipGraph as it is."""

    def __init__(self, scene, device):
        self.device = torch.device(device)
        self.cfg = SimpleNamespace(num_layers=1)
        self.hq, self.hkv, self.D = scene.Hq, HKV, scene.D
        self.dtype = BF
        self.scale = scene.scale
        self.table = scene.table().to(self.device)
        self._keep = {}
        self.kept = None  # every row's attention output of the last forward

    def __call__(self, ids, meta, kv_caches):
        hq, hkv, D = self.hq, self.hkv, self.D
        qkv = ops.embed_rows(self.table, ids)
        T = qkv.shape[0]
        kc, vc = kv_caches[0]
        k = qkv[:, hq * D:(hq + hkv) * D].view(T, hkv, D)
        v = qkv[:, (hq + hkv) * D:].view(T, hkv, D)
        ops.kv_write(k, v, kc, vc, meta.slots)
        # NaN first: a row no kernel writes is seen
        out = torch.full((T, hq * D), float("nan"), dtype=BF, device=qkv.device)
        out = paged_attention(qkv, kc, vc, meta, hq, hkv, D, self.scale, out)
        keep = self._keep.get(T)
        if keep is None:  # first met outside a capture: the runner warms a bucket up before it captures
            keep = self._keep[T] = torch.empty_like(out)
        keep.copy_(out)
        self.kept = keep
        if meta.logits_idx is not None:
            return ops.gather_rows(out, meta.logits_idx)
        return out

    def logits(self, h, gather=True, dtype=None):
        return h

    def greedy(self, h):
        return h.float().argmax(dim=-1).to(torch.int32)


# ------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------
@dataclass
class Res:
    si: object
    rows: list       # the runner's [(Sequence, row)]
    ret: object      # what execute() returned (CPU tensor or None)
    kept: torch.Tensor  # [T, Hq, D] bf16 (CPU): every row's output
    index: list      # per row (PSeq, position)
    want_rows: list  # [(Sequence, row)]: the last row of each item that ends its sequence's pending tokens
    seqs: list       # the Sequence objects, in item order
    host_ids: np.ndarray  # the ids prepare() made on the host


class Driver:
    """Real Sequence objects over block tables from a shuffled permutation of the block ids
    1 .. NB - 1, stepped through runner.prepare() / runner.execute().  Keeps the image the cache
    must have: NaN but for the slots of the (key group, position) pairs run so far."""

    def __init__(self, scene, device="cpu", use_graphs=False, seed=11, spare=3):
        self.scene = scene
        self.model = ProbeModel(scene, device)
        nblk = [(scene.K[g].shape[0] - scene.shared[g] + BS - 1) // BS for g in range(len(scene.K))]
        NB = 1 + sum(nblk) + spare
        self.runner = ModelRunner(self.model, block_size=BS, max_model_len=MAX_MODEL_LEN, num_blocks=NB,
                                  use_graphs=use_graphs)
        assert self.runner.num_blocks == NB and self.runner.max_blocks == 288
        self.runner.kv.fill_(float("nan"))
        gen = torch.Generator().manual_seed(seed)
        perm = (1 + torch.randperm(NB - 1, generator=gen)).tolist()
        self.blocks, p = [], 0
        for g in range(len(scene.K)):
            head = self.blocks[scene.base[g]][: scene.shared[g] // BS] if scene.shared[g] else []
            self.blocks.append(head + perm[p:p + nblk[g]])
            p += nblk[g]
        shape = (NB, HKV, BS, scene.D)
        self.kimg = torch.full(shape, float("nan"), dtype=BF)
        self.vimg = torch.full(shape, float("nan"), dtype=BF)

    def sequence(self, it):
        s, st, n = it.seq, it.start, it.n
        assert s.q_from <= st and st + n <= s.n
        table = list(self.blocks[s.kg][: (st + n + BS - 1) // BS])
        if it.mode == "prefill":
            plen = it.plen or st + n
            return Sequence(list(s.ids[:plen]), SamplingParams(), block_table=table, num_computed=st)
        if it.mode == "decode":
            assert n == 1
            return Sequence(list(s.ids[:st]), SamplingParams(), output_ids=[s.ids[st]], block_table=table,
                            num_computed=st)
        if it.mode == "inflight":
            assert n == 1 and st > 0 and it.row >= 0
            return Sequence(list(s.ids[:st]), SamplingParams(), block_table=table, num_computed=st,
                            num_inflight=1, inflight_row=it.row)
        assert it.mode == "extend" and n > 1
        return Sequence(list(s.ids[:st]), SamplingParams(), output_ids=list(s.ids[st:st + n]),
                        block_table=table, num_computed=st)

    def step(self, items):
        r = self.runner
        seqs = [self.sequence(it) for it in items]
        ritems = [(s, it.start, it.n) for s, it in zip(seqs, items)]
        fly = [it for it in items if it.mode == "inflight"]
        if fly:  # the previous step's device ids: ours at the rows named, id 0 elsewhere
            prev = torch.zeros(max(it.row for it in fly) + 3, dtype=torch.int32)
            for it in fly:
                prev[it.row] = it.seq.ids[it.start]
            r.prev_ids = prev.to(r.device)
        si, rows = r.prepare(ritems)
        host_ids = np.array(si.ids)  # before execute(): on the CPU the device ids are this very array
        ret = r.execute(si)
        # row order of a step: prefill chunks, then decode rows, each in item order
        dec = [r._as_decode(*x) for x in ritems]
        order = [i for i, d in enumerate(dec) if not d] + [i for i, d in enumerate(dec) if d]
        index, want_rows = [], []
        for i in order:
            it = items[i]
            index += [(it.seq, p) for p in range(it.start, it.start + it.n)]
            if it.mode != "prefill" or it.plen is None or it.plen == it.start + it.n:
                want_rows.append((seqs[i], len(index) - 1))
        T = len(index)
        # a replayed graph wrote the static buffer of its bucket; an eager step the last forward's
        kept = self.model._keep[si.decode_graph] if si.decode_graph else self.model.kept
        kept = kept[:T].cpu().view(T, self.scene.Hq, self.scene.D).clone()
        for it in items:
            self.wrote(it.seq.kg, it.start, it.n)
        return Res(si, rows, None if ret is None else ret.cpu(), kept, index, want_rows, seqs, host_ids)

    def wrote(self, kg, start, n):
        sc = self.scene
        for p in range(start, start + n):
            blk, off = self.blocks[kg][p // BS], p % BS
            self.kimg[blk, :, off] = sc.K[kg][p]
            self.vimg[blk, :, off] = sc.V[kg][p]

    # ---- the checks
    def want(self, res):
        out, i = [], 0
        while i < len(res.index):  # runs of consecutive positions of one sequence
            s, a = res.index[i]
            j = i + 1
            while j < len(res.index) and res.index[j] == (s, a + j - i):
                j += 1
            out.append(self.scene.want(s, a, a + j - i))
            i = j
        return torch.cat(out)

    def check_rows(self, res, what):
        """(a) every row against its float64 answer; (c) the rows that feed the LM head."""
        want = self.want(res)
        try:
            check(self.scene.kind, res.kept, want, what)
        except AssertionError as e:
            raise AssertionError(f"{e} -- rows are (sequence, position): "
                                 f"{self._name_rows(res, res.kept, want)}") from None
        rows = [row for _, row in res.want_rows]
        assert res.si.logits_rows.tolist() == rows, f"{what}: logits_rows"
        pairs = zip(res.rows, res.want_rows)
        assert len(res.rows) == len(rows) and all(a is b and i == j for (a, i), (b, j) in pairs), \
            f"{what}: the (sequence, row) pairs"
        if rows:
            assert res.ret is not None and res.ret.shape[0] == len(rows), f"{what}: returned rows"
            sel = res.kept.reshape(len(res.index), -1)[rows]
            assert torch.equal(res.ret.view(torch.int16), sel.view(torch.int16)), \
                f"{what}: the returned rows are not the last row of each finished item"
        else:
            assert res.ret is None

    def _name_rows(self, res, got, want):
        x = torch.nan_to_num(excess(self.scene.kind, got, want), nan=float("inf")).flatten(1).amax(dim=1)
        bad = torch.nonzero(x > 1).flatten().tolist()
        return ", ".join(f"row {r} = ({res.index[r][0].name}, {res.index[r][1]})" for r in bad[:6]) + \
            (f" and {len(bad) - 6} more" if len(bad) > 6 else "")

    def check_cache(self, what):
        """(b) the slots of every (key group, position) run so far hold its K / V bit for bit; every
        other slot, block 0 included, is still NaN."""
        for name, got, img in (("K", self.runner.kv[0, 0], self.kimg), ("V", self.runner.kv[0, 1], self.vimg)):
            got = got.cpu()
            nan = torch.isnan(img)
            assert bool(nan[0].all())
            if not torch.equal(torch.isnan(got), nan):
                d = torch.nonzero(torch.isnan(got) != nan)[0].tolist()
                raise AssertionError(f"{what}: {name} cache: slot (block {d[0]}, kv head {d[1]}, offset {d[2]}) is "
                                     f"{'NaN but was run' if not bool(nan[tuple(d)]) else 'written but was never run'}")
            same = got.view(torch.int16)[~nan] == img.view(torch.int16)[~nan]
            if not bool(same.all()):
                d = torch.nonzero((got.view(torch.int16) != img.view(torch.int16)) & ~nan)[0].tolist()
                raise AssertionError(f"{what}: {name} cache: slot (block {d[0]}, kv head {d[1]}, offset {d[2]}), "
                                     f"channel {d[3]} holds another token's row")

    def run(self, items, what, cache=True):
        res = self.step(items)
        self.check_rows(res, what)
        if cache:
            self.check_cache(what)
        return res


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


# ------------------------------------------------------------------------------------------------
# the cases: what the GPU tests run (and, at the contexts given, the CPU reference run)
# ------------------------------------------------------------------------------------------------
CHUNKS = (100, 7, 193)           # the 300-token sequence: chunk starts 100 and 107
COMPANY = ((33, 129, 64), (17, 200), (1, 65, 96))  # whole prefills that share its three steps
BATCHES = (1, 3, 16, 64, 256)    # B * Hkv = 2, 6, 32, 128, 512: splits 128, 128, 256, 512, 2048
GRAPH_BATCHES = {3: ([1, 129, 4097], [16, 17, 2048], [255, 33, 2100]),
                 5: ([15, 128, 257, 2049, 97], [31, 32, 96, 127, 2047], [15, 4097, 129, 16, 2100])}
EXTENDS = ((30, 2), (127, 5), (250, 16))  # (start, n): contexts 31-32, 128-132, 251-266
MIXED_CTX = (1, 17, 129, 257, 2049)
INFLIGHT_CTX = (17, 129, 31, 2049, 257)
INFLIGHT_ROWS = (3, 0, 6, 1, 4)  # their rows in the previous step's ids: another order, with gaps


SETUP_CHUNK = 512


def setup_chunks(n):
    return [(a, min(SETUP_CHUNK, n - a)) for a in range(0, n, SETUP_CHUNK)]


def prefill_steps(jobs):
    """[(sequence, start, n)] -> steps of prefill chunks, a sequence at most SETUP_CHUNK tokens a step."""
    steps = []
    for s, st, n in jobs:
        for j, (a, c) in enumerate(setup_chunks(n)):
            while len(steps) <= j:
                steps.append([])
            steps[j].append(It(s, st + a, c, plen=st + n))
    return steps


def split_of(B):
    return max(ops.decode_split_size(B, HKV), BS)


def prefill_needles(n):
    return P.needle_positions(n, 64, BS)


def copies(scene, L):
    return (len(L) + scene.G - 1) // scene.G if scene.kind == "N" else 1


def plan_prefill(scene):
    """Steps of the chunked and batched prefill case: [[It]]."""
    A = scene.seq("A", scene.keys(300), needles=prefill_needles(300))
    steps, st = [], 0
    for c, others in zip(CHUNKS, COMPANY):
        items = [It(A, st, c, plen=300)]
        for n in others:
            items.append(It(scene.seq(f"p{n}", scene.keys(n), needles=prefill_needles(n)), 0, n))
        items.insert(1, items.pop(0))  # the chunk is not the step's first sequence
        steps.append(items)
        st += c
    first, second = [], []
    for ql, past in P.PREFILL_QP:
        s = scene.seq(f"qp{ql}+{past}", scene.keys(ql + past), needles=prefill_needles(ql + past))
        if past:
            first.append(It(s, 0, past, plen=ql + past))
        second.append(It(s, past, ql))
    return steps + [first, second]


def plan_prefix_hit(scene):
    a = scene.keys(100)
    A = scene.seq("A", a, needles=prefill_needles(100))
    B = scene.seq("B", scene.keys(150, base=a, shared=64), q_from=64, needles=prefill_needles(150))
    return [[It(A, 0, 100)], [It(B, 64, 86)]]


def plan_contexts(scene, ctxs, tag="c"):
    """One key group and its writer per context; the steps that prefill them all, a sequence at
    most SETUP_CHUNK tokens a step."""
    w = {n: scene.seq(f"{tag}{n}", scene.keys(n), needles=prefill_needles(n)) for n in ctxs}
    return w, prefill_steps([(s, 0, n) for n, s in w.items()])


def decode_copy(scene, writer, t, split, k_start=0, tag="d"):
    """Copy t of the decode row of ``writer``'s context: its last position, asked again."""
    n = writer.n
    L = P.needle_positions(n, split, BS, k_start)
    return scene.seq(f"{tag}{n}.{t}", writer.kg, n, q_from=n - 1, needles=L, rot=t % copies(scene, L))


def _contexts(scene, ctxs, w):
    """The writers of the contexts: made here (with the steps that prefill them) or given."""
    if w is None:
        return plan_contexts(scene, ctxs)
    return w, []


def plan_decode(scene, ctxs, batches=BATCHES, w=None):
    """Every batch size over every context: {B: [[It]]}, batches of B rows that walk the contexts,
    a context's rows repeating it as decode copies 0, 1, ..."""
    w, setup = _contexts(scene, ctxs, w)
    plan = {}
    for B in batches:
        met = {n: 0 for n in ctxs}
        nb = max(1, -(-len(ctxs) // B))
        plan[B] = []
        for b in range(nb):
            items = []
            for i in range(B):
                n = ctxs[(b * B + i) % len(ctxs)]
                items.append(It(decode_copy(scene, w[n], met[n], split_of(B), tag=f"d{B}."), n - 1, 1, "decode"))
                met[n] += 1
            plan[B].append(items)
    return setup, plan


def plan_graph_decode(scene, batches=None, w=None):
    batches = GRAPH_BATCHES if batches is None else batches
    ctxs = sorted({n for bs in batches.values() for b in bs for n in b})
    w, setup = _contexts(scene, ctxs, w)
    plan = {}
    for B, lists in batches.items():
        plan[B] = [[It(decode_copy(scene, w[n], t + i, split_of(B), tag=f"g{B}.{t}."), n - 1, 1, "decode")
                    for i, n in enumerate(ctx)] for t, ctx in enumerate(lists)]
    return setup, plan


def plan_extend(scene, extends=EXTENDS):
    setup, items = [], []
    for st, n in extends:
        s = scene.seq(f"e{st}+{n}", scene.keys(st + n), needles=prefill_needles(st + n))
        setup.append(It(s, 0, st, plen=st))
        items.append(It(s, st, n, "extend"))
    return [setup], items


def plan_mixed(scene, ctxs=MIXED_CTX, w=None):
    w, setup = _contexts(scene, ctxs, w)
    setup = setup or [[]]
    A = scene.seq("A", scene.keys(90), needles=prefill_needles(90))
    C = scene.seq("C", scene.keys(70), needles=prefill_needles(70))
    setup[0].append(It(A, 0, 40, plen=90))
    dec = [It(decode_copy(scene, w[n], i, split_of(len(ctxs))), n - 1, 1, "decode") for i, n in enumerate(ctxs)]
    # decode rows among the prefill chunks: the runner sorts them behind
    return setup, [dec[0], It(C, 0, 70), dec[1], dec[2], It(A, 40, 50), dec[3], dec[4]]


def plan_inflight(scene, ctxs=INFLIGHT_CTX, rows=INFLIGHT_ROWS, w=None):
    w, setup = _contexts(scene, ctxs, w)
    items = [It(decode_copy(scene, w[n], i, split_of(len(ctxs)), tag="f"), n - 1, 1, "inflight", row=r)
             for i, (n, r) in enumerate(zip(ctxs, rows))]
    return setup, items


def cascade_rows(S):
    """(contexts, shared blocks of each row's table, the shared_len the runner must choose) of the
    cascade batches: per number S of shared leading blocks the tails of attn_probes (the first row's
    context is shared + 1); and one batch whose rows share 18 blocks but for a 40-key row of the
    prefix itself, whose (40 - 1) // 16 = 2 clamps the run to 32 keys."""
    return [S * BS + t for t in P.CASCADE_TAILS], S * BS if S >= 2 else 0


CLAMP_CTX, CLAMP_SHARED = 40, 32


def plan_cascade(scene, prefixes=P.CASCADE_PREFIX_BLOCKS):
    """{label: (shared_len, [[It]] batches of decode copies)}, the setup steps."""
    base = scene.keys(18 * BS)
    Wb = scene.seq("base", base, needles=prefill_needles(18 * BS))
    setup0, jobs = [It(Wb, 0, 18 * BS)], []
    split = split_of(len(P.CASCADE_TAILS))
    assert split == split_of(8) == 128
    plan, writers = {}, {}
    for S in prefixes:
        ctxs, shared = cascade_rows(S)
        ws = []
        for n in ctxs:
            kg = scene.keys(n, base=base if S else None, shared=S * BS)
            s = scene.seq(f"s{S}.{n}", kg, q_from=S * BS, needles=prefill_needles(n))
            ws.append(s)
            jobs.append((s, S * BS, n - S * BS))
        writers[S] = ws
        Ls = [P.needle_positions(w.n, split, BS, shared) for w in ws]
        nt = max(copies(scene, L) for L in Ls)
        plan[f"{S} shared blocks"] = (shared, [
            [It(decode_copy(scene, w, t, split, shared, tag=f"k{S}."), w.n - 1, 1, "decode") for w in ws]
            for t in range(nt)])
    if 18 in prefixes:
        ws = writers[18][1:]
        L = P.needle_positions(CLAMP_CTX, split, BS, CLAMP_SHARED)
        short = scene.seq("base40", base, CLAMP_CTX, q_from=CLAMP_CTX - 1, needles=L, rot=0)
        plan["clamped"] = (CLAMP_SHARED, [
            [It(decode_copy(scene, w, 0, split, CLAMP_SHARED, tag="kc."), w.n - 1, 1, "decode") for w in ws[:2]]
            + [It(short, CLAMP_CTX - 1, 1, "decode")]
            + [It(decode_copy(scene, w, 1, split, CLAMP_SHARED, tag="kc."), w.n - 1, 1, "decode") for w in ws[2:]]])
    return [setup0] + prefill_steps(jobs), plan


# ------------------------------------------------------------------------------------------------
# RTOL_W_STEP
# ------------------------------------------------------------------------------------------------
def w_shapes():
    """Every shape the W probe runs at in tests/test_step_attention_gpu.py, as ("decode", context,
    split, k_start) or ("prefill", first row, rows, 0): W's keys and queries depend on the position
    alone, so a shape is its key count and plan."""
    out = set()
    for B in BATCHES:
        out |= {("decode", n, split_of(B), 0) for n in P.DECODE_CTX}
    for B, lists in GRAPH_BATCHES.items():
        out |= {("decode", n, split_of(g), 0) for ctx in lists for n in ctx
                for g in (B, 4 if B == 3 else 8)}
    for st, n in EXTENDS:  # alone (eager rows n, graph bucket) and together
        for g in (n, 2 if n == 2 else 8 if n == 5 else 16, sum(e[1] for e in EXTENDS), 24):
            out |= {("decode", p + 1, split_of(g), 0) for p in range(st, st + n)}
        out.add(("prefill", st, n, 0))  # as a flash chunk
        out.add(("prefill", 0, st, 0))
    for n in MIXED_CTX + INFLIGHT_CTX:
        out |= {("decode", n, split_of(5), 0), ("decode", n, split_of(8), 0)}
    for S in P.CASCADE_PREFIX_BLOCKS:
        ctxs, shared = cascade_rows(S)
        out |= {("decode", n, 128, shared) for n in ctxs}
        out |= {("decode", n, 128, 0) for n in ctxs}  # the replays of the graph with shared_len 0
        out |= {("prefill", S * BS + a, c, 0) for n in ctxs for a, c in setup_chunks(n - S * BS)}
    out |= {("decode", n, 128, CLAMP_SHARED) for n in cascade_rows(18)[0][1:] + [CLAMP_CTX]}
    out |= {("decode", n, 128, 4 * BS) for n in cascade_rows(3)[0][2:]}  # the shared_len mutation, which W passes
    out.add(("prefill", 0, 18 * BS, 0))
    # whole prefills (the setups of the decode cases included) and chunks
    whole = set(P.DECODE_CTX) | {n for c in COMPANY for n in c} | {100, 70}
    whole |= {n for lists in GRAPH_BATCHES.values() for ctx in lists for n in ctx}
    whole |= set(MIXED_CTX) | set(INFLIGHT_CTX)
    out |= {("prefill", a, c, 0) for n in whole for a, c in setup_chunks(n)}
    st = 0
    for c in CHUNKS:
        out.add(("prefill", st, c, 0))
        st += c
    out |= {("prefill", 0, 40, 0), ("prefill", 40, 50, 0), ("prefill", 64, 86, 0)}
    for ql, past in P.PREFILL_QP:
        out.add(("prefill", past, ql, 0))
        if past:
            out.add(("prefill", 0, past, 0))
    return sorted(out)


def measure_rtol_w_step(Ds=(128, 64)):
    """Worst relative error of attn_probes.emulate() against the float64 answer over w_shapes(), at
    G = 1 (W asks the same of every head of a group): (error, where)."""
    worst = (0.0, "")
    for D in Ds:
        sc = Scene("W", 1, D)
        kg = sc.keys(max(s[1] + (s[2] if s[0] == "prefill" else 0) for s in w_shapes()))
        K, V = sc.K[kg], sc.V[kg]
        q1 = sc._q(1, 0, (), None)
        for what, a, b, k0 in w_shapes():
            if what == "decode":
                n = a
                q, mask = q1, torch.ones(1, n, dtype=torch.bool)
                plans, defers = [P.decode_plan(n, b, k0)], (0.0,)
            else:
                n = a + b
                q = q1.expand(b, -1, -1)
                mask = torch.arange(n)[None, :] <= torch.arange(a, n)[:, None]
                plans, defers = [P.prefill_plan(n)], (0.0, 8.0)
            want = P.exact_attention(q, K[:n], V[:n], mask, sc.scale)[0]
            for plan in plans:
                for defer in defers:
                    got = P.emulate(q, K[:n], V[:n], mask, sc.scale, plan, defer)[0].double()
                    nz = want != 0
                    assert bool((got[~nz] == 0).all())
                    e = float(((got - want).abs()[nz] / want.abs()[nz]).max())
                    if e > worst[0]:
                        worst = (e, f"{what} {(a, b, k0)} D {D} defer {defer}")
    return worst
