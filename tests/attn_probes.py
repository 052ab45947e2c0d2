"""Structured attention inputs whose float64 answer pins the weight of every single key.

i.i.d. random Q / K / V make a long attention row an average of many random V rows: a kernel
that drops, doubles or misplaces one key moves the output by less than the tolerance a bf16
kernel needs.  The probes here are built so that one key is a visible share of the output:

U "count"      K = 0: every visible key weighs exactly 1 / n.  V[j, (j + 7 kvh) % D] = 1, so
               output channel d = (visible keys of residue class d) / (visible keys).
N "needle"     every (query row, head) asks for ONE key and gets its V row to a bf16 ulp: the
               score of the needle is about 40 nat above every other key.
W "weighted"   q = 8 e_0, K[j, 0] = base[(j // 32 + kvh) % 5] + ((37 j) % 29) / 32: neighbouring
               chunks, waves, splits and the cascade prefix have different maxima.  V as in U.
S "staircase"  causal prefill: scores constant inside a 64-key tile, the tile maxima walk around
               the threshold of the deferred running max.  V as in U.

All inputs are exact in bf16 (asserted), the expected output is a float64 softmax attention over
the same values, so the only error of a kernel is its own rounding.

The needle.  A head of a GQA group of one has one query per kv head, far fewer than the places
where an index can go wrong (both sides of every split, block, chunk and tile boundary, key 0,
the last key, k_start).  So a key is not found by a one-hot channel per needle but by its
position written in binary: K[j, off + b] = +1 / -1 by bit b of j (13 bits, off = 5 kvh) and the
query is c times the code of the key it wants.  The wanted key scores 13 c, every other key at
most 11 c, and c = 16 floor(20 / (16 scale)) makes the gap 2 c scale about 40 nat.  Any key can
be a needle for any query: decode rows are repeated (sharing their cache blocks) until every
listed position has been asked for, and each prefill row walks the listed positions it can see
plus its own diagonal.

Plain torch on the CPU; the GPU tests import this module as a sibling.
"""
import math
from dataclasses import dataclass, field

import torch

LOG2E = 1.4426950408889634
BF = torch.bfloat16

# --- tolerances -------------------------------------------------------------------------------
# |got - want| <= rtol * |want| + floor, elementwise.  No probe needs a floor: an expected zero
# is a channel without a visible key, whose V entries are exact zeros, and every other expected
# element is compared relative to itself (bf16 and the f32 accumulators are floating point).
FLOOR = 0.0
# U: the kernel's answer is an exact quotient (P = 1, counts exact in f32) rounded once or twice:
# two bf16 half-ulps.
RTOL_U = 2.0 ** -7
# N: one bf16 ulp of the expected element (see ulp()); the other keys weigh e^-39.
ULPS_N = 1.0
# W, S: twice the worst relative error of emulate() -- flash arithmetic on the CPU: per 32- or
# 64-key chunk max, exp2 in f32, P rounded to bf16 before PV, f32 accumulation, bf16 output -- against
# the float64 answer, over every shape of tests/test_attention_exact_gpu.py (decode and cascade at the
# splits 128 and 2048, prefill, the q_past shards; S with the max deferred by up to 8 and not at
# all).  The factor 2 covers exp2f and the accumulation order, which the emulation does not model.
# Measured by measure_rtol() (tests/test_attn_probes_cpu.py asserts the constants are 2 x what it
# measures, rounded up in the third digit): W 0.708 % (prefill, a query row over 128 keys, D 128),
# S 0.384 % (790 keys, not deferred).
RTOL_W = 2 * 0.00708
RTOL_S = 2 * 0.00384

DECODE_CTX = [1, 15, 16, 17, 31, 32, 33, 96, 97, 127, 128, 129, 255, 257, 2047, 2048, 2049, 2100, 4097]
CASCADE_TAILS = [1, 16, 17, 129, 2049]
CASCADE_PREFIX_BLOCKS = [0, 1, 3, 18]
PREFILL_QP = [(1, 0), (31, 1), (33, 5), (64, 0), (65, 63), (100, 0), (128, 64), (257, 40), (64, 700)]
ENCODER_LENS = [1, 7, 63, 64, 65, 128, 300]
# prefill over more than 128 cache blocks (the flash kernel keeps a sequence's first 128 block-table
# entries in registers and reads the rest from memory): 134 blocks of 8 keys, 134 and 268 of 16 and 8
LONG_QP = [(70, 1000), (40, 2100)]
# staircase: (q_len, past) over 790 and 832 keys = 13 tiles, the last one partial / full; the query
# rows of the first see from 1 key to all of them
STAIR_QP = [(790, 0), (100, 732)]
# key shards of a context-parallel rank as (keys in the shard, q_len, q_past): q_past negative for
# part of the rows, zero, inside the keys, past all keys, and so negative that no row sees a key
SHARD_GEOM = [(200, 96, -40), (130, 70, 0), (300, 65, 100), (77, 40, 500), (64, 33, -33), (129, 1, 128)]

S_STEPS = [6, 6, 6, 7.5, 8.5, -30, 20, 6, 6, 7.5, 8.5, -20]
W_BASE = [0.0, 1.5, -2.0, 3.0, -1.0]
NEEDLE_BITS = 13


def ulp(x):
    """Spacing of bf16 at |x| (float64 tensor): 2^(floor(log2 |x|) - 7); 0 at 0."""
    _, e = torch.frexp(x.abs())
    return torch.where(x == 0, torch.zeros_like(x), torch.ldexp(torch.ones_like(x), e - 8))


def tolerance(kind, want):
    want = want.double()
    if kind == "N":
        return ULPS_N * ulp(want) + FLOOR
    rtol = {"U": RTOL_U, "W": RTOL_W, "S": RTOL_S}[kind]
    return rtol * want.abs() + FLOOR


def excess(kind, got, want):
    """|got - want| / tolerance, elementwise (inf where an expected zero is not an exact zero);
    got passes where this is <= 1."""
    d = (got.double() - want.double()).abs()
    t = tolerance(kind, want)
    inf = torch.full_like(d, float("inf"))
    return torch.where(t > 0, d / t.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), inf))


def check(kind, got, want, what=""):
    assert torch.isfinite(got.double()).all(), f"{what}: non-finite output"
    x = excess(kind, got, want)
    if bool((x > 1).any()):
        i = int(x.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), x.shape))
        raise AssertionError(f"{what}: probe {kind}: {int((x > 1).sum())} of {x.numel()} elements off; worst at "
                             f"{idx}: got {float(got.double().flatten()[i])!r}, want "
                             f"{float(want.double().flatten()[i])!r} ({float(x.flatten()[i]):.3g} x tolerance)")


def exact_attention(q, k, v, mask, scale):
    """float64 softmax attention.  q [R, Hq, D], k / v [n, Hkv, D], mask bool [R, n] (True =
    visible).  Returns (o f64 [R, Hq, D], zero for a row without a visible key; lse2 f64 [R, Hq]:
    log2 of the sum of exp of the scores, -inf for such a row)."""
    R, Hq, D = q.shape
    n, Hkv, _ = k.shape
    g = Hq // Hkv
    s = torch.einsum("rhgd,nhd->hgrn", q.double().view(R, Hkv, g, D), k.double()).reshape(Hq, R, n) * scale
    s = s.masked_fill(~mask[None], float("-inf"))
    m = s.amax(dim=-1, keepdim=True) if n else torch.full((Hq, R, 1), float("-inf"), dtype=torch.float64)
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.exp(s - m0)
    l = p.sum(dim=-1, keepdim=True)
    o = torch.einsum("hgrn,nhd->rhgd", (p / l.clamp_min(1e-300)).view(Hkv, g, R, n), v.double()).reshape(R, Hq, D)
    lse2 = (m0 + torch.log(l)).squeeze(-1).T * LOG2E
    return o, lse2


@dataclass
class Probe:
    kind: str
    Hkv: int
    G: int
    D: int
    scale: float
    causal: bool
    k: list  # per sequence [n, Hkv, D] bf16
    v: list
    seq: list  # batch row -> sequence
    q: list  # per batch row [q_len, Hq, D] bf16
    past: list  # per batch row: position of its first query relative to its first key
    _cache: dict = field(default_factory=dict)

    @property
    def Hq(self):
        return self.Hkv * self.G

    @property
    def B(self):
        return len(self.q)

    def n(self, r):
        return self.k[self.seq[r]].shape[0]

    def qlen(self, r):
        return self.q[r].shape[0]

    def hi(self, r):
        """Visible keys of each query row: keys [0, hi) (may be <= 0)."""
        n, ql = self.n(r), self.qlen(r)
        if not self.causal:
            return torch.full((ql,), n, dtype=torch.long)
        return (self.past[r] + 1 + torch.arange(ql)).clamp(max=n)

    def mask(self, r):
        return torch.arange(self.n(r))[None, :] < self.hi(r)[:, None]

    def _exact(self, r):
        if r not in self._cache:
            s = self.seq[r]
            self._cache[r] = exact_attention(self.q[r], self.k[s], self.v[s], self.mask(r), self.scale)
        return self._cache[r]

    def want(self, r):
        return self._exact(r)[0]

    def lse2(self, r):
        return self._exact(r)[1]

    def want_all(self):
        return torch.cat([self.want(r) for r in range(self.B)])

    def rows_of_seq(self, s):
        return [r for r in range(self.B) if self.seq[r] == s]


def _bf16_exact(*ts):
    out = []
    for t in ts:
        b = t.to(BF)
        assert torch.equal(b.double(), t.double()), "probe value not exact in bf16"
        out.append(b)
    return out


def _onehot_v(n, Hkv, D):
    v = torch.zeros(n, Hkv, D)
    j = torch.arange(n)
    for h in range(Hkv):
        v[j, h, (j + 7 * h) % D] = 1.0
    return v


def decode_geom(ctx):
    return [(n, 1, n - 1) for n in ctx]


def prefill_geom(pairs):
    return [(ql + past, ql, past) for ql, past in pairs]


def build_U(geom, Hkv, G, D, causal=True):
    k, v, q = [], [], []
    for n, ql, _ in geom:
        kk, vv, qq = _bf16_exact(torch.zeros(n, Hkv, D), _onehot_v(n, Hkv, D), torch.ones(ql, Hkv * G, D))
        k.append(kk), v.append(vv), q.append(qq)
    return Probe("U", Hkv, G, D, 1 / math.sqrt(D), causal, k, v, list(range(len(geom))), q, [g[2] for g in geom])


def build_W(geom, Hkv, G, D, causal=True):
    k, v, q = [], [], []
    base = torch.tensor(W_BASE)
    for n, ql, _ in geom:
        kk = torch.zeros(n, Hkv, D)
        j = torch.arange(n)
        for h in range(Hkv):
            kk[:, h, 0] = base[(j // 32 + h) % 5] + ((37 * j) % 29) / 32.0
        qq = torch.zeros(ql, Hkv * G, D)
        qq[:, :, 0] = 8.0
        kk, vv, qq = _bf16_exact(kk, _onehot_v(n, Hkv, D), qq)
        k.append(kk), v.append(vv), q.append(qq)
    return Probe("W", Hkv, G, D, 1 / math.sqrt(D), causal, k, v, list(range(len(geom))), q, [g[2] for g in geom])


def stair_levels(ntiles):
    lv = [0.0]
    for t in range(1, ntiles):
        lv.append(lv[-1] + S_STEPS[(t - 1) % len(S_STEPS)])
    return torch.tensor(lv)


def build_S(geom, Hkv, G, D):
    """scale = ln 2 and q = e_0, so a score is K[j, 0] in log2 units: the level of the key's tile."""
    k, v, q = [], [], []
    for n, ql, _ in geom:
        kk = torch.zeros(n, Hkv, D)
        kk[:, :, 0] = stair_levels((n + 63) // 64)[torch.arange(n) // 64][:, None]
        qq = torch.zeros(ql, Hkv * G, D)
        qq[:, :, 0] = 1.0
        kk, vv, qq = _bf16_exact(kk, _onehot_v(n, Hkv, D), qq)
        k.append(kk), v.append(vv), q.append(qq)
    return Probe("S", Hkv, G, D, math.log(2.0), True, k, v, list(range(len(geom))), q, [g[2] for g in geom])


def needle_positions(n, split=128, BS=16, k_start=0, tile=64):
    """The keys of an n-key row where an index can go wrong: key 0, the last key, both sides of
    every split boundary (counted from k_start, which includes k_start - 1 and k_start), of a
    cache-block boundary (the first and the last one), of a 32-key chunk and of a 64-key tile."""
    p = {0, n - 1}
    for edge in range(k_start, n + 1, split):
        p |= {edge - 1, edge}
    last_block = (n - 1) // BS * BS
    for edge in (BS, last_block, k_start + 32, k_start + tile, 32, tile):
        p |= {edge - 1, edge}
    return sorted(x for x in p if 0 <= x < n)


def _code(j, D, h):
    """[len(j), D]: position j in binary, +1 / -1, in channels 5 h .. 5 h + 12."""
    c = torch.zeros(len(j), D)
    bits = (j[:, None] >> torch.arange(NEEDLE_BITS)[None, :]) & 1
    c[:, 5 * h: 5 * h + NEEDLE_BITS] = (2 * bits - 1).float()
    return c


def build_N(geom, Hkv, G, D, needles, causal=True, seed=3, shared_prefix=0):
    """needles[i]: the listed positions of row i of geom.  A one-query row is repeated until each
    of them has been asked for by some head of each kv head; a longer row asks, per query row and
    head, for one of the listed positions it sees or for its last visible key, in rotation.
    ``shared_prefix``: the first keys of every sequence are those of sequence 0 (a cascade prefix)."""
    assert 5 * (Hkv - 1) + NEEDLE_BITS <= D
    gen = torch.Generator().manual_seed(seed)
    scale = 1 / math.sqrt(D)
    c = 16.0 * math.floor(20.0 / scale / 16.0)
    k, v, q, seq, past = [], [], [], [], []
    for s, ((n, ql, pst), L) in enumerate(zip(geom, needles)):
        assert n < (1 << NEEDLE_BITS) and all(0 <= x < n for x in L)
        kk = torch.stack([_code(torch.arange(n), D, h) for h in range(Hkv)], dim=1)
        vv = torch.randint(1, 256, (n, Hkv, D), generator=gen) / 64.0
        vv = vv * (2.0 * torch.randint(0, 2, (n, Hkv, D), generator=gen) - 1.0)
        kk, vv = _bf16_exact(kk, vv)
        if s and shared_prefix:
            vv[:shared_prefix] = v[0][:shared_prefix]
        k.append(kk), v.append(vv)
        if ql == 1:
            for t in range((len(L) + G - 1) // G):
                want = torch.tensor([[L[(t * G + g + 3 * h) % len(L)] for g in range(G)] for h in range(Hkv)])
                qq = torch.stack([c * _code(want[h], D, h) for h in range(Hkv)]).reshape(1, Hkv * G, D)
                q.append(_bf16_exact(qq)[0]), seq.append(s), past.append(pst)
            continue
        qq = torch.zeros(ql, Hkv * G, D)
        for i in range(ql):
            hi = min(n, pst + i + 1) if causal else n
            if hi <= 0:
                continue
            cand = [x for x in L if x < hi] + [hi - 1]
            for h in range(Hkv):
                want = torch.tensor([cand[(i + g + 3 * h) % len(cand)] for g in range(G)])
                qq[i, h * G:(h + 1) * G] = c * _code(want, D, h)
        q.append(_bf16_exact(qq)[0]), seq.append(s), past.append(pst)
    return Probe("N", Hkv, G, D, scale, causal, k, v, seq, q, past)


def build(kind, geom, Hkv, G, D, causal=True, split=128, BS=16, k_start=0):
    if kind == "U":
        return build_U(geom, Hkv, G, D, causal)
    if kind == "W":
        return build_W(geom, Hkv, G, D, causal)
    if kind == "S":
        return build_S(geom, Hkv, G, D)
    return build_N(geom, Hkv, G, D, [needle_positions(n, split, BS, k_start) for n, _, _ in geom], causal,
                   shared_prefix=k_start)


# --- the paged cache ----------------------------------------------------------------------------
def to_paged(probe, BS, seed=5, extra_width=0, shared_blocks=0):
    """K / V caches [NB, Hkv, BS, D] filled through a shuffled block permutation, the block table
    [B, width] (rows of one sequence share its blocks) and the context lengths.  Slots past a
    sequence's last key and three spare blocks hold NaN: a kernel must not let them in, not even
    under a zero weight.  Table entries past a row's blocks name a valid but wrong block: the
    first block of the next sequence.  ``shared_blocks``: every row's first table entries are
    those of sequence 0 (a cascade prefix, which must hold the same keys in every sequence)."""
    gen = torch.Generator().manual_seed(seed)
    nblk = [(kk.shape[0] + BS - 1) // BS for kk in probe.k]
    for kk, vv in zip(probe.k, probe.v):
        m = shared_blocks * BS
        assert torch.equal(kk[:m], probe.k[0][:m]) and torch.equal(vv[:m], probe.v[0][:m])
    NB = sum(nblk) + 3
    kc = torch.full((NB, probe.Hkv, BS, probe.D), float("nan"), dtype=BF)
    vc = torch.full_like(kc, float("nan"))
    perm = torch.randperm(NB, generator=gen).tolist()
    blocks, p = [], 0
    for s, (kk, vv) in enumerate(zip(probe.k, probe.v)):
        blocks.append(perm[p:p + nblk[s]])
        p += nblk[s]
        for i, blk in enumerate(blocks[s]):
            m = min(BS, kk.shape[0] - i * BS)
            kc[blk, :, :m] = kk[i * BS:i * BS + m].transpose(0, 1)
            vc[blk, :, :m] = vv[i * BS:i * BS + m].transpose(0, 1)
    width = max(nblk) + extra_width
    bt = torch.zeros(probe.B, width, dtype=torch.int32)
    for r in range(probe.B):
        s = probe.seq[r]
        bt[r] = blocks[(s + 1) % len(blocks)][0]
        bt[r, :nblk[s]] = torch.tensor(blocks[s], dtype=torch.int32)
        bt[r, :shared_blocks] = torch.tensor(blocks[0][:shared_blocks], dtype=torch.int32)
    ctx = torch.tensor([probe.n(r) for r in range(probe.B)], dtype=torch.int32)
    return kc, vc, bt, ctx


# --- flash arithmetic on the CPU -----------------------------------------------------------------
def decode_plan(n, split, k_start=0):
    """Key chunks as the decode kernel walks them: per split of the keys past k_start, four waves
    taking the 32-key chunks w, w + 4, ...; the cascade prefix [0, k_start) in 64-key tiles."""
    plan = []
    if k_start:
        plan.append([(a, min(a + 64, k_start)) for a in range(0, k_start, 64)])
    for s0 in range(k_start, n, split):
        s1 = min(s0 + split, n)
        chunks = [(a, min(a + 32, s1)) for a in range(s0, s1, 32)]
        plan += [chunks[w::4] for w in range(4) if chunks[w::4]]
    return plan


def prefill_plan(n):
    return [[(a, min(a + 64, n)) for a in range(0, n, 64)]]


def emulate(q, k, v, mask, scale, plan, defer=0.0):
    """Flash arithmetic: every group of the plan runs an online softmax over its chunks (chunk
    max; the running max moves only when it grows by more than ``defer``; exp2 in f32; P rounded
    to bf16 for PV; f32 accumulation), the groups are merged by their (max, sum), the output is
    rounded to bf16.  Returns (o bf16 [R, Hq, D], m + log2(l) f32 [R, Hq])."""
    R, Hq, D = q.shape
    g = Hq // k.shape[1]
    kf = k.float().repeat_interleave(g, dim=1)
    vf = v.float().repeat_interleave(g, dim=1)
    s = torch.einsum("rhd,nhd->hrn", q.float(), kf) * torch.tensor(scale * LOG2E, dtype=torch.float32)
    s = s.masked_fill(~mask[None], float("-inf"))
    ninf = torch.tensor(float("-inf"))
    parts = []
    for chunks in plan:
        m = torch.full((Hq, R), float("-inf"))
        l = torch.zeros(Hq, R)
        o = torch.zeros(Hq, R, D)
        for a, b in chunks:
            sc = s[:, :, a:b]
            m_new = torch.maximum(m, sc.amax(dim=-1))
            m_new = torch.where(m_new > m + defer, m_new, m)
            base = torch.where(m_new == ninf, torch.zeros_like(m_new), m_new)
            alpha = torch.exp2(m - base)
            e = torch.exp2(sc - base[..., None])
            l = l * alpha + e.sum(dim=-1)
            o = o * alpha[..., None] + torch.einsum("hrn,nhd->hrd", e.to(BF).float(), vf[a:b])
            m = m_new
        parts.append((m, l, o))
    M = torch.stack([p[0] for p in parts]).amax(dim=0)
    M0 = torch.where(M == ninf, torch.zeros_like(M), M)
    L = sum(torch.exp2(p[0] - M0) * p[1] for p in parts)
    O = sum(torch.exp2(p[0] - M0)[..., None] * p[2] for p in parts)
    out = torch.where(L[..., None] > 0, O / L.clamp_min(1e-38)[..., None], torch.zeros_like(O))
    return out.permute(1, 0, 2).to(BF), (M0 + torch.log2(L)).T


def emulate_seq(probe, s, split=None, k_start=0, defer=0.0):
    """The batch rows of sequence s (they share keys and mask) through emulate(): the decode plan
    when ``split`` is given, else prefill.  Returns (o, lse2, want) over those rows, concatenated."""
    rows = probe.rows_of_seq(s)
    n = probe.k[s].shape[0]
    plan = decode_plan(n, split, k_start) if split else prefill_plan(n)
    if len(rows) > 1:
        assert all(probe.qlen(r) == 1 for r in rows)
    q = torch.cat([probe.q[r] for r in rows])
    o, lse = emulate(q, probe.k[s], probe.v[s], probe.mask(rows[0]).expand(q.shape[0], n), probe.scale, plan, defer)
    return o, lse, torch.cat([probe.want(r) for r in rows])


def shapes(kinds=("U", "N", "W", "S"), Gs=(1, 2, 4, 8), Ds=(64, 128)):
    """Every (label, probe, split, k_start, defers) of tests/test_attention_exact_gpu.py that goes
    through emulate(); the encoder shapes (D 32 included) are listed apart, under G = 1.  U, W and
    S give every head of a group the same query, so their answer at G = 1 is their answer at every
    G and they are listed at G = 1 alone; N is listed at every G."""
    for D in Ds:
        for G in Gs:
            for kind in kinds:
                if kind != "N" and G != 1:
                    continue
                if kind == "S":
                    if D == 128:
                        yield f"stair G{G} D{D}", build_S(prefill_geom(STAIR_QP), 2, G, D), None, 0, (0.0, 8.0)
                    continue
                for split in (128, 2048):
                    yield (f"decode {kind} G{G} D{D} split{split}",
                           build(kind, decode_geom(DECODE_CTX), 2, G, D, split=split), split, 0, (0.0,))
                    for S in CASCADE_PREFIX_BLOCKS:
                        geom = decode_geom([S * 16 + t for t in CASCADE_TAILS])
                        yield (f"cascade {kind} G{G} D{D} split{split} prefix{S}",
                               build(kind, geom, 2, G, D, split=split, k_start=S * 16), split, S * 16, (0.0,))
                yield (f"prefill {kind} G{G} D{D}", build(kind, prefill_geom(PREFILL_QP), 2, G, D), None, 0,
                       (0.0, 8.0))
                if D == 128 and G in (1, 4):
                    yield (f"prefill long {kind} G{G} D{D}", build(kind, prefill_geom(LONG_QP), 2, G, D), None, 0,
                           (0.0, 8.0))
                if kind != "N" and D == 128:
                    yield f"shards {kind}", build(kind, SHARD_GEOM, 2, 4, D), None, 0, (0.0,)
    for D in (32, 64, 128):
        for kind in kinds:
            if kind in ("U", "N") and 1 in Gs:
                geom = [(n, n, 0) for n in ENCODER_LENS]
                yield f"encoder {kind} D{D}", build(kind, geom, 4, 1, D, causal=False), None, 0, (0.0,)


def measure_rtol(kinds=("W", "S")):
    """Worst relative error of emulate() against the float64 answer per probe kind, over shapes()."""
    worst = {}
    for label, probe, split, k0, defers in shapes(kinds):
        for sq in range(len(probe.k)):
            for defer in defers:
                got, _, want = emulate_seq(probe, sq, split, k0, defer)
                got, nz = got.double(), want != 0
                assert bool((got[~nz] == 0).all()), label
                if nz.any():
                    e = float(((got - want).abs()[nz] / want.abs()[nz]).max())
                    if e > worst.get(probe.kind, (0.0, ""))[0]:
                        worst[probe.kind] = (e, f"{label} sequence {sq} ({probe.k[sq].shape[0]} keys) defer {defer}")
    return worst


# --- mutants: wrong answers a broken kernel would give ------------------------------------------
def _parts(probe, r, cfg):
    """Key ranges the kernels merge: the cascade prefix and the splits past it."""
    n, split, k0 = probe.n(r), cfg["split"], cfg.get("k_start", 0)
    return ([(0, k0)] if k0 else []) + [(a, min(a + split, n)) for a in range(k0, n, split)]


def _answer(probe, r, k=None, v=None, mask=None):
    s = probe.seq[r]
    k = probe.k[s] if k is None else k
    v = probe.v[s] if v is None else v
    return exact_attention(probe.q[r], k, v, mask, probe.scale)[0]


def _pad_blocks(t, BS):
    n = t.shape[0]
    pad = (-n) % BS
    return torch.cat([t, torch.zeros(pad, *t.shape[1:], dtype=t.dtype)]) if pad else t


def _swap_blocks(t, a, b, BS):
    n = t.shape[0]
    p = _pad_blocks(t, BS).clone()
    p[a * BS:(a + 1) * BS], p[b * BS:(b + 1) * BS] = p[b * BS:(b + 1) * BS].clone(), p[a * BS:(a + 1) * BS].clone()
    return p[:n]


def mutate(name, probe, r, cfg):
    """(wrong answer f64 [q_len, Hq, D], altered bool [q_len]) of batch row r under mutant
    ``name``, or None where the mutant does not apply to the row.  cfg: BS, split, k_start."""
    s = probe.seq[r]
    k, v, mask, hi = probe.k[s], probe.v[s], probe.mask(r), probe.hi(r)
    n, ql, BS, k0 = probe.n(r), probe.qlen(r), cfg["BS"], cfg.get("k_start", 0)
    seen = hi > 0

    def drop(lo, up, alt):  # keys [lo, up) per query row, where alt
        cols = torch.arange(n)[None, :]
        gone = (cols >= lo[:, None]) & (cols < up[:, None]) & alt[:, None]
        return _answer(probe, r, mask=mask & ~gone), alt & (gone & mask).any(dim=1)

    if name == "drop the last visible key":
        return drop(hi - 1, hi, seen)
    if name == "drop a middle key":
        return drop(hi // 2, hi // 2 + 1, hi >= 3)
    if name == "one stale key after the last":
        alt = hi == n
        # a stale slot: the K row of key 0 under a V row that is not the sequence's (channels rolled by one)
        k2, v2 = torch.cat([k, k[:1]]), torch.cat([v, v[:1].roll(1, dims=-1)])
        return _answer(probe, r, k2, v2, torch.cat([mask, alt[:, None]], dim=1)), alt
    if name == "drop the last partial block":
        return drop(hi - hi % BS, hi, (hi % BS != 0) & seen)
    if name in ("drop the last split", "drop a middle split"):
        ns = (hi - k0 + cfg["split"] - 1) // cfg["split"]
        which = ns - 1 if name == "drop the last split" else (ns - 1) // 2
        lo = k0 + which * cfg["split"]
        return drop(lo, lo + cfg["split"], ns >= 2)
    if name == "drop the cascade prefix":
        return drop(torch.zeros(ql, dtype=torch.long), torch.full((ql,), k0), seen & (k0 > 0)) if k0 else None
    if name == "merge ignoring the maxima":
        parts = _parts(probe, r, cfg)
        if len(parts) < 2:
            return None
        num, den = 0.0, 0.0
        for a, b in parts:
            cols = torch.arange(n)[None, :]
            o, lse2 = exact_attention(probe.q[r], k, v, mask & (cols >= a) & (cols < b), probe.scale)
            # the sum relative to the part's own maximum: 2^(lse2 - max)
            sc = torch.einsum("rhd,nhd->rhn", probe.q[r].double(), k[a:b].double().repeat_interleave(probe.G, 1))
            sc = (sc * probe.scale * LOG2E).masked_fill(~mask[:, None, a:b], float("-inf"))
            mx = sc.amax(dim=-1)
            l = torch.where(torch.isinf(mx), torch.zeros_like(mx), torch.exp2(lse2 - mx))
            num, den = num + l[..., None] * o, den + l
        return num / den.clamp_min(1e-300)[..., None], (hi > parts[0][1]) & seen
    if name in ("causal mask off by +1", "causal mask off by -1"):
        if not probe.causal:
            return None
        d = 1 if name.endswith("+1") else -1
        h2 = (hi + d).clamp(max=n)
        return _answer(probe, r, mask=torch.arange(n)[None, :] < h2[:, None]), h2.clamp(min=0) != hi.clamp(min=0)
    if name.startswith("swap V blocks") or name.startswith("swap K blocks"):
        a, b = {"0,1": (0, 1), "0,8": (0, 8)}[name[-3:]]
        if n <= b * BS:
            return None
        if name[5] == "V":
            return _answer(probe, r, v=_swap_blocks(v, a, b, BS), mask=mask), seen
        return _answer(probe, r, k=_swap_blocks(k, a, b, BS), mask=mask), seen
    if name == "read the other kv head":
        return _answer(probe, r, k.flip(1), v.flip(1), mask), seen
    if name == "the next row's block table":
        if len(probe.k) < 2:
            return None
        t = (s + 1) % len(probe.k)

        def fit(x):  # the other sequence's first n keys; past its end the table holds nothing of ours
            pad = torch.zeros(max(0, n - x.shape[0]), *x.shape[1:], dtype=x.dtype)
            return torch.cat([x[:n], pad])

        k2, v2 = fit(probe.k[t]), fit(probe.v[t])
        return _answer(probe, r, k2, v2, mask), seen
    if name == "k_start one block late":
        if not cfg.get("cascade"):
            return None
        return drop(torch.full((ql,), k0), torch.full((ql,), k0 + BS), hi > k0)
    if name == "k_start one block early":
        if not cfg.get("cascade") or k0 < BS:
            return None
        k2, v2 = torch.cat([k, k[k0 - BS:k0]]), torch.cat([v, v[k0 - BS:k0]])
        return _answer(probe, r, k2, v2, torch.cat([mask, mask[:, k0 - BS:k0]], dim=1)), hi > k0 - BS
    raise KeyError(name)


MUTANTS = ["drop the last visible key", "drop a middle key", "one stale key after the last",
           "drop the last partial block", "drop the last split", "drop a middle split", "drop the cascade prefix",
           "merge ignoring the maxima", "causal mask off by +1", "causal mask off by -1", "swap V blocks 0,1",
           "swap V blocks 0,8", "swap K blocks 0,1", "read the other kv head", "the next row's block table",
           "k_start one block late", "k_start one block early"]
