"""Structured inputs for the xGMI collectives (csrc/xgmi_allreduce.hip, K14) whose answer pins, per
element, which ranks were read there, in which order they were added and how the sum was rounded.

The pinned semantics: every all-reduce form adds the ranks' bf16 values in float32, in rank order
0, 1, .., world - 1, into an accumulator that starts at +0.0f, and rounds the sum ONCE to bf16
(nearest, ties to even).  So all ranks -0.0 give +0.0, inf + (-inf) gives NaN, subnormal sums are
not flushed.  The fused forms round twice more: res = bf16(bf16(sum) + res), then RMSNorm(res) * w
with the slicing and the roundings of rmsnorm_kernel.

Two references, which tests/test_ar_probes_cpu.py shows to agree on every probe:
  ref64(xs)          the float64 sum (from +0.0) rounded once to bf16 -- for the probes built so
                     that the sum is exact in any order;
  emu_allreduce(xs)  float32 adds in rank order from +0.0f, one round-to-nearest-even -- where the
                     order or the rounding is the point.
Every comparison of an all-reduce, a gather or a residual is bit for bit (NaN meets NaN, +0 is not
-0); only the fused forms' normalised output is compared under row_probes' "rms" limit, which was
measured for rmsnorm_kernel, whose thread slicing and reduction order the fused kernels share.

Every probe is a function of (world, ...) and returns the per-rank inputs xs[r] and the answer.
``emu_*(.., mutant=)`` injects ONE fault; the CPU test shows that each is rejected by a probe.
Plain torch: neither the package's GPU code nor torch.distributed is imported."""
import functools
import itertools

import torch

import row_probes as R
from row_probes import BF, SENTINEL  # noqa: F401

WORLDS = (2, 3, 8)
BLOCKS = 32     # LK_XGMI_AR_BLOCKS of the GPU tests = kArSlices of the plain kernels
THREADS = 512   # kArThreads
GUARD = 64      # SENTINEL elements behind a plain result (the fused forms: one row)
# the smallest sizes at which each index expression of the plain one-shot / gather kernels can go
# wrong: one vector, one short / full / just-over block, one vector past 32 full blocks, three
# thread-stride rounds with an odd rest
PLAIN_N = (8, 8 * 511, 8 * 512, 8 * 513, 8 * (32 * 512 + 1), 8 * (3 * 32 * 512 + 17))
FUSED_H = 512
FUSED_T = (1, 31, 32, 33, 65)  # fewer rows than blocks, one per block, uneven rows per block
WIDE_T = 5                     # at every width of row_probes.NORM_H
TINY = 2.0 ** -133             # spacing of the bf16 subnormals

MUTANTS = ("drop", "twice", "rotate", "bf16_acc", "trunc", "half_up", "skip_round", "off32", "block_off",
           "row_off", "owner_floor", "no_clamp", "stale")
NEEDS_WORLD_3 = ("rotate", "bf16_acc")  # two addends have one order and one rounding


def two_shot_T(world):
    """Fewer rows than owners, one each, one more, the last owners short or empty, more rows per
    owner than workgroups."""
    out = []
    for T in (1, world - 1, world, world + 1, world + 1 + world, 33 * world + 1):
        if T not in out:
            out.append(T)
    return tuple(out)


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 62)
    g = torch.Generator()
    g.manual_seed(seed)
    return g


# =============================================================================== comparisons
def bits(t):
    return t.contiguous().view(torch.int16)


def mismatch(got, want):
    """Per element: the bf16 bit patterns differ (NaN meets any NaN)."""
    g, w = got.to(BF), want.to(BF)
    return (bits(g) != bits(w)) & ~(torch.isnan(g) & torch.isnan(w))


def verdict(name, got, want, kind="E"):
    """One result row (name, ok, first bad index, got, want).  ``got`` is the WHOLE buffer the call
    wrote into; ``want`` answers its leading part and everything behind it must hold SENTINEL."""
    g = got.detach().cpu().reshape(-1)
    w = want.detach().cpu()
    n = w.numel()
    if g.numel() < n:
        return (name, False, -1, float(g.numel()), float(n))
    if kind == "E":
        b = mismatch(g[:n], w.reshape(-1))
    else:
        b = R.bad(kind, g[:n].view(w.shape), w).reshape(-1)
    b = torch.cat([b, g[n:].double() != SENTINEL])
    if not bool(b.any()):
        return (name, True, -1, 0.0, 0.0)
    i = int(b.nonzero()[0])
    return (name, False, i, float(g[i]), float(w.reshape(-1)[i]) if i < n else SENTINEL)


def guarded(n, device="cpu", guard=GUARD, dtype=BF):
    """-> (buf of n + guard SENTINELs, its leading n elements)."""
    buf = torch.full((n + guard,), SENTINEL, dtype=dtype, device=device)
    return buf, buf[:n]


def ref64(xs):
    """The float64 sum from +0.0, rounded once to bf16."""
    acc = torch.zeros(xs[0].shape, dtype=torch.float64)
    for x in xs:
        acc = acc + x.double()
    return R.to_bf16(acc).to(BF)


# =============================================================================== probes
def layout(world, n, seed=0):
    """Rank r gives 2^r * bit(r, i), the bits from a seeded generator (no period in i): the sum, at
    most 255, is exact in bf16 in any order and names the ranks that were read at element i.  Rank
    r's bits do not depend on the world size."""
    b = torch.randint(0, 2, (8, n), generator=_gen(n, seed, 77))[:world]
    sh = torch.arange(world)[:, None]
    return [(b[r] << r).to(BF) for r in range(world)], (b << sh).sum(0).to(BF)


def order(world, n):
    """(2^24, 1, -2^24) on ranks a < b < c, zeros elsewhere, (a, b, c) cycling over all rank triples:
    f32 addition in rank order gives (2^24 + 1 = 2^24) - 2^24 = +0; any order that does not add a and b
    first gives 1."""
    assert world >= 3
    trip = torch.tensor(list(itertools.combinations(range(world), 3)))
    i = torch.arange(n)
    t = trip[i % trip.shape[0]]
    x = torch.zeros(world, n)
    x[t[:, 0], i] = 2.0 ** 24
    x[t[:, 1], i] = 1.0
    x[t[:, 2], i] = -(2.0 ** 24)
    return [R.exact_bf16(x[r]) for r in range(world)], torch.zeros(n, dtype=BF)


_INF = float("inf")
# (addends in rank order on the chosen ranks, the answer); the rest of the ranks give +0.0
ROUNDING_CASES = (
    ((256.0, 1.0), 256.0),            # a tie, to even: truncation agrees, round-half-up gives 258
    ((258.0, 1.0), 260.0),            # a tie, to even: truncation gives 258
    ((-256.0, -1.0), -256.0),
    ((-258.0, -1.0), -260.0),
    ((_INF, -_INF), float("nan")),    # not +-inf
    ((-_INF, _INF), float("nan")),
    ((3 * TINY, 5 * TINY), 8 * TINY),             # subnormal + subnormal, subnormal
    ((100 * TINY, 100 * TINY), 200 * TINY),       # subnormal + subnormal, normal
    ((-7 * TINY, 64 * TINY), 57 * TINY),
    ((256.0, 1.0, 1.0), 258.0),       # one f32 sum; bf16 pairwise adds give 256
    ((-256.0, -1.0, -1.0), -258.0),
    (None, 0.0),                      # every rank -0.0: +0.0, the accumulator starts at +0.0
)


def rounding(world, n):
    """The cases of ROUNDING_CASES along the element index (those of three addends from world 3 on),
    their ranks cycling over all rank pairs / triples -> (xs, want, case index per element)."""
    cases = [c for c in ROUNDING_CASES if c[0] is None or len(c[0]) <= world]
    i = torch.arange(n)
    k = i % len(cases)
    x = torch.zeros(world, n, dtype=torch.float64)
    want = torch.zeros(n, dtype=torch.float64)
    for ci, (add, ans) in enumerate(cases):
        sel = i[k == ci]
        want[sel] = ans
        if add is None:
            x[:, sel] = -0.0
            continue
        combos = torch.tensor(list(itertools.combinations(range(world), len(add))))
        ranks = combos[(sel // len(cases)) % combos.shape[0]]
        for j, a in enumerate(add):
            x[ranks[:, j], sel] = a
    return [x[r].to(BF) for r in range(world)], want.to(BF), k


@functools.lru_cache(maxsize=2)
def _fused_pool(H):
    """The rows of row_probes in the order they are dealt: a residual-tie row, the double-rounding
    row (None), a dense row, the last spike, the eps-dominated row, .. -> [(x row, residual row)]."""
    xn, ns = R.norm_rows(H)
    xr, rr = R.resid_rows(H)
    zero = torch.zeros(H, dtype=BF)
    nrm = lambda j: (xn[j], zero)  # noqa: E731
    res = lambda j: (xr[j], rr[j])  # noqa: E731
    first = [res(0), None, nrm(ns), nrm(ns - 1), nrm(ns + 4), res(1), nrm(ns + 3), res(2), nrm(0), res(3),
             nrm(ns + 1), nrm(ns + 2)]
    return first + [nrm(j) for j in range(1, ns - 1)]


def fused(world, H, T, seed=0):
    """T rows of row_probes (norm_rows with a zero residual, resid_rows with theirs) and one
    double-rounding row (row 1: sum +-257, residual +-1), split over the ranks: the element's value
    on a random rank, from world 3 on an exactly cancelling pair +-p (p an integer below 128) on two
    other random ranks, zeros elsewhere -- every partial sum is exact in f32, in any order.
    -> dict(xs, res, w, sum (bf16), want_res (bf16), want_out (float64))."""
    pool = _fused_pool(H)
    g = _gen(world, H, T, seed)
    v = torch.zeros(T, H, dtype=torch.float64)
    e = torch.zeros(T, H, dtype=torch.float64)
    res = torch.zeros(T, H, dtype=torch.float64)
    dbl = torch.zeros(T, dtype=torch.bool)
    for t in range(T):
        row = pool[t % len(pool)]
        if row is None:
            s = 1.0 - 2.0 * torch.randint(0, 2, (H,), generator=g).double()
            v[t], e[t], res[t], dbl[t] = 256 * s, s, s, True
        else:
            v[t], res[t] = row[0].double(), row[1].double()
    N = T * H
    p = torch.randint(1, 128, (N,), generator=g).double()
    isd = dbl[:, None].expand(T, H).reshape(N)
    c = torch.zeros(N, world, dtype=torch.float64)
    c[:, 0] = v.reshape(N)
    c[:, 1] = e.reshape(N)
    if world >= 3:
        c[:, 1] = torch.where(isd, c[:, 1], p)
        c[:, 2] = torch.where(isd, c[:, 2], -p)
    if world >= 4:
        c[:, 2] = torch.where(isd, p, c[:, 2])
        c[:, 3] = torch.where(isd, -p, c[:, 3])
    perm = torch.rand(N, world, generator=g).argsort(1)
    x = torch.zeros(N, world, dtype=torch.float64).scatter_(1, perm, c)
    xs = [R.exact_bf16(x[:, r].reshape(T, H), "xs") for r in range(world)]
    w = R.gamma(H)
    total = R.to_bf16(v + e)  # 257 -> 256
    want_res = R.add64(total, res)
    return dict(xs=xs, res=R.exact_bf16(res, "residual"), w=w, sum=total.to(BF), want_res=want_res.to(BF),
                want_out=R.rms64(want_res, w), dbl=dbl)


# =============================================================================== emulations
def _store(acc, mutant=None):
    """f32 -> bf16 as the kernels' f2bf; 'trunc' truncates, 'half_up' rounds ties toward +inf."""
    if mutant == "trunc":
        return R.round_store(acc, "trunc")
    if mutant == "half_up":
        a = acc.double()
        fin = torch.isfinite(a)
        z = torch.where(fin, a, torch.zeros_like(a))
        u = R.ulp(z).clamp_min(R.BF_TINY)
        return torch.where(fin, torch.floor(z / u + 0.5) * u, a).to(BF)
    return acc.to(BF)


def plain_blocks(n):
    """(workgroups, vectors per workgroup) of the plain one-shot and gather kernels."""
    nv = n // 8
    blocks = min(BLOCKS, max(1, (nv + THREADS - 1) // THREADS))
    return blocks, (nv + blocks - 1) // blocks


def _sum32(xs, mutant=None, rank=0, prev=None):
    """The unrounded f32 accumulator as rank ``rank`` computes it.  The mutants that misplace a
    read hit the LAST rank's staged copy (indices wrap)."""
    world = len(xs)
    src = [x.reshape(-1).float() for x in xs]
    n = src[0].numel()
    last = world - 1
    if mutant == "off32":
        src[last] = torch.roll(src[last], -32)
    if mutant == "block_off":
        src[last] = torch.roll(src[last], -8 * plain_blocks(n)[1])
    if mutant == "row_off":
        src[last] = torch.roll(src[last], -xs[0].shape[-1])
    if mutant == "stale":
        src[last] = prev[last].reshape(-1).float()
    seq = list(range(world))
    if mutant == "rotate":
        seq = seq[rank:] + seq[:rank]
    if mutant == "drop":
        seq.remove(last)
    if mutant == "twice":
        seq.insert(1, 0)
    acc = torch.zeros(n)
    for r in seq:
        acc = acc + src[r]
        if mutant == "bf16_acc":
            acc = acc.to(BF).float()
    return acc.view(xs[0].shape)


def emu_allreduce(xs, mutant=None, rank=0, prev=None):
    """The one-shot all-reduce on rank ``rank``: f32 adds in rank order from +0.0f, one RNE store.
    ``prev``: the inputs of the call before (mutant 'stale')."""
    return _store(_sum32(xs, mutant, rank, prev), mutant)


def _owner_rows(T, world, mutant=None):
    """Row ranges [ra, rb) the two-shot kernel reduces and gathers, owner by owner."""
    n = T // world if mutant == "owner_floor" else (T + world - 1) // world
    out = []
    for o in range(world):
        ra, rb = o * n, (o + 1) * n
        if mutant != "no_clamp":
            ra, rb = min(T, ra), min(T, rb)
        out.append((ra, rb))
    return out


def _scatter_rows(buf, rows, T, H, ranges):
    """Write rows[ra:rb] into the flat buffer; rows past T (mutant 'no_clamp') are sums of nothing,
    zeros, and land behind the result as far as the buffer reaches."""
    for ra, rb in ranges:
        for row in range(ra, rb):
            lo, hi = row * H, min((row + 1) * H, buf.numel())
            if lo >= hi:
                continue
            buf[lo:hi] = rows[row, : hi - lo] if row < T else 0.0
    return buf


def emu_allreduce2(xs, mutant=None, rank=0, prev=None, guard=GUARD):
    """The two-shot all-reduce of xs[r] [T, H], in place on rank ``rank`` -> the flat buffer of
    T * H + guard elements (the guard SENTINEL): rows no owner covers keep the rank's input."""
    T, H = xs[0].shape
    red = emu_allreduce(xs, mutant, rank, prev)
    buf, view = guarded(T * H, guard=guard)
    view.copy_(xs[rank].reshape(-1))
    return _scatter_rows(buf, red, T, H, _owner_rows(T, len(xs), mutant))


def emu_fused(xs, res, w, eps=R.NORM_EPS, mutant=None, rank=0, prev=None, two_shot=False):
    """All-reduce + residual + RMSNorm -> (residual buffer, out buffer), each [T + 1, H] flat with
    the last row a SENTINEL guard (the residual's rows start as ``res``, out's as SENTINEL):
    x = bf16(f32 sum), res = bf16(x + res), out = rmsnorm_kernel's arithmetic on res."""
    T, H = xs[0].shape
    s = _sum32(xs, mutant, rank, prev)
    x = s if mutant == "skip_round" else _store(s, mutant).float()
    new = _store(x + res.float(), mutant)
    y = R.emu_rms(new, w, eps)
    rbuf, rview = guarded(T * H, guard=H)
    rview.copy_(res.reshape(-1))
    obuf, _ = guarded(T * H, guard=H)
    ranges = _owner_rows(T, len(xs), mutant) if two_shot else [(0, T)]
    return _scatter_rows(rbuf, new, T, H, ranges), _scatter_rows(obuf, y, T, H, ranges)
