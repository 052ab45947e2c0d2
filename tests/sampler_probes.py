"""A CPU model of the token selectors of csrc/sampling.hip that says which token a given (engine seed,
request seed, position) must produce, and the inputs the exact sampler tests run.

Nothing here touches the GPU; numpy only.

The random stream is modelled bit for bit: ``hash3`` is the kernels' splitmix avalanche in uint64 and
``uniform`` their float32 expression ``min(((h >> 8) + 0.5) * 2^-24, 1 - 2^-24)``.  Everything after
the draw is float64:

``order``    the candidates of a row by (value desc, id asc), -0.0 == +0.0, -inf never a candidate
``chain``    sample_topkp_kernel: e = exp((v - v0) / T) over ``order``, the top-p and min-p prefix,
             the first kept candidate whose inclusive prefix exceeds u * kept mass
``gumbel``   select_kernel: argmax of l / T - log(-log u) per id, ties to the lowest id

and each returns the ADMISSIBLE SET of tokens.  A comparison the kernel makes in float32 (a top-p
boundary, a min-p boundary, a prefix against u, the best Gumbel score against the next) is ambiguous
when its sides lie within ``eps`` relative of each other; an ambiguous comparison admits both outcomes,
any other admits one.  A row is PINNED when its set has one member.  ``exact=True`` is for rows whose
kept values are all equal (e = 1 or 0, integer prefixes): no comparison is ambiguous there, and u * kept
and top_p * total are rounded to float32 as the kernel rounds them.

EPS and EPS_G are twice the worst relative error of a float32 emulation of the kernels' order of
operations (``measure_eps``, ``measure_eps_g``) against float64 over the random inputs below; the
factor 2 is for __expf / __logf and FMA contraction, which the emulation does not model (the margin
of row_probes.py).  tests/test_sampler_probes_cpu.py asserts that the constants are what it measures,
and docs/kernels.md ("Sampler") carries the derivation.

``mut`` names a deliberate mistake in the model (MUTANTS); tests/test_sampler_probes_cpu.py shows that
each changes the expected token of a probe row, i.e. that the GPU tests would catch the same mistake
in a kernel."""
import functools

import numpy as np

F32 = np.float32
U64 = np.uint64
KMAX, KCAND, THREADS = 1024, 4096, 1024  # kSampKMax, kCand, kSampThreads
U_CAP = F32(1.0 - 2.0 ** -24)            # 0x1.fffffep-1f
M32 = 0xFFFFFFFF
NINF = float("-inf")

# Measured (measure_eps over random_cases() and radix_rows(), measure_eps_g over the Gumbel rows), rounded up in the
# third digit: the inclusive prefix of up to 1024 float32 terms (6 shuffle levels + up to 15 serial
# wave sums), e of a rounded difference times a rounded 1 / T, and one more rounding for top_p * total
# and u * kept; the Gumbel score's two nested logarithms, the product and the sum.
MEASURED = {"eps": 5.35e-7, "eps_g": 2.84e-7}
EPS = 2 * MEASURED["eps"]
EPS_G = 2 * MEASURED["eps_g"]
E_FLOOR = 0.01  # e below it is compared with no min_p of the random cases (min_p >= 0.05)

MUTANTS = ("topp_lt", "pick_ge", "pos_mod_w", "row_hash", "zero_order", "drop_wave1", "k_unclamped")

# (h >> 8) == 0xFFFFFF, where (h + 0.5) * 2^-24 rounds to 1.0f: found by search_u1_*()
U1_GUMBEL = ((123, 0, 21265, 905), (0x1234567890, 3, 263, 1898), ((1 << 62) + 12345, 1, 2720, 1595))  # (seed, row, step, id)
U1_SAMPLE = ((123, 22885348, 3), (0x1234567890, 7788311, 0), (0x5DEECE66D, 2220608, 21))            # (seed, rseed, hl)
# u * 1024 an integer in float32 (a prefix of a 1024-wide plateau EQUALS u): ">" against ">="
INT_U_1024 = ((123, 1976, 0), (123, 14043, 0), (0x1234567890, 3153, 0))                               # (seed, rseed, hl)


# ------------------------------------------------------------------------------------ the stream
def fold(seed):
    """(unsigned)(seed ^ (seed >> 32)) of the 63-bit seed ops passes down."""
    seed = int(seed) & ((1 << 63) - 1)
    return (seed ^ (seed >> 32)) & M32


def _u64(x):
    return (np.atleast_1d(np.asarray(x)).astype(np.int64) & M32).astype(U64)


def hash3(a, b, c):
    """The kernels' hash3 on the low 32 bits of a, b, c (broadcast), uint32."""
    a, b, c = _u64(a), _u64(b), _u64(c)
    with np.errstate(over="ignore"):
        x = (a << U64(32)) ^ (b * U64(0x9E3779B97F4A7C15)) ^ c
        x = x ^ (x >> U64(30))
        x = x * U64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> U64(27))
        x = x * U64(0x94D049BB133111EB)
        x = x ^ (x >> U64(31))
    return (x >> U64(32)).astype(np.uint32)


def uniform(h, cap=True):
    """The kernels' u in float32; ``cap=False`` is the expression before the fix (u == 1 possible)."""
    u = ((np.asarray(h, np.uint32) >> np.uint32(8)).astype(F32) + F32(0.5)) * F32(2.0 ** -24)
    return np.minimum(u, U_CAP) if cap else u


def sample_hash(seed, rseed, hl, row=0, mut=()):
    a = fold(seed) + (row if "row_hash" in mut else 0)
    return hash3(a, rseed, hl)


def gumbel_hash(seed, row, step, ids):
    return hash3(fold(seed) + int(row), step, ids)


def search_u1_sample(seed, hl, n=1 << 26):
    """Request seeds below n whose draw at (seed, hl) has (h >> 8) == 0xFFFFFF (how U1_SAMPLE was found)."""
    out = []
    for lo in range(0, n, 1 << 22):
        r = np.arange(lo, min(lo + (1 << 22), n))
        out += r[(hash3(fold(seed), r, hl) >> np.uint32(8)) == 0xFFFFFF].tolist()
    return out


def search_u1_gumbel(seed, row, V, steps):
    """(step, id) with id < V whose Gumbel draw has (h >> 8) == 0xFFFFFF (how U1_GUMBEL was found)."""
    ids = np.arange(V)
    for step in range(steps):
        hit = np.flatnonzero((gumbel_hash(seed, row, step, ids) >> np.uint32(8)) == 0xFFFFFF)
        if len(hit):
            return step, int(hit[0])
    return None


def search_int_u(seed, hl, n, width=1024):
    """Request seeds below n for which float32(u * width) is an integer."""
    r = np.arange(n)
    u = uniform(sample_hash(seed, r, hl)) * F32(width)
    return r[u == np.floor(u)].tolist()


# ------------------------------------------------------------------------------------ parameters
def prm_rows(B, width=8, temp=0.8, top_k=40, top_p=0.9, min_p=0.0, pen=1.0, last_n=64, slots=None, reset=0,
             seeds=None):
    """int32 [B, width] parameter rows of lk_sample; every argument a scalar or one value per row."""
    prm = np.zeros((B, width), dtype=np.int32)
    f = prm.view(F32)
    f[:, 0], f[:, 1], f[:, 2] = temp, top_p, pen
    prm[:, 3], prm[:, 4] = top_k, last_n
    prm[:, 5] = np.arange(B) if slots is None else slots
    prm[:, 6] = reset
    prm[:, 7] = np.arange(B) if seeds is None else seeds
    if width == 12:
        f[:, 8] = min_p
    else:
        assert np.all(np.asarray(min_p) == 0)
    return prm


def parse(row):
    row = np.ascontiguousarray(row, dtype=np.int32)
    f = row.view(F32)
    return dict(temp=f[0], top_p=f[1], pen=f[2], top_k=int(row[3]), last_n=int(row[4]), slot=int(row[5]),
                reset=int(row[6]), rseed=int(row[7]), min_p=f[8] if len(row) == 12 else F32(0))


def k_of(temp, top_k, V, mut=()):
    if temp <= 0:
        return 1
    k = min(top_k if top_k > 0 else KMAX, V)
    return k if "k_unclamped" in mut else min(k, KMAX)


def penalize(l, pen, tokens):
    """The repeat penalty in float32 on each unique token of the window, as the kernel applies it."""
    l = np.array(l, dtype=F32)
    for t in sorted({int(t) for t in tokens if 0 <= int(t) < len(l)}):
        l[t] = l[t] / F32(pen) if l[t] > 0 else l[t] * F32(pen)
    return l


def window(hist_row, hl, last_n, W):
    n = min(hl, last_n if last_n > 0 else W, W)
    return [int(hist_row[(hl - 1 - j) % W]) for j in range(n)]


# ------------------------------------------------------------------------------------ the model
def _fkey(v):
    """The sampler's order-preserving key BEFORE the fix: -0.0 below +0.0."""
    b = np.asarray(v, F32).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, ~b & M32, b | 0x80000000)


def order(l, K, mut=()):
    """ids of the K largest entries by (value desc, id asc); -0.0 == +0.0; -inf never a candidate, so
    fewer than K ids when fewer entries are finite."""
    l = np.asarray(l, F32)
    ids = np.flatnonzero(l > NINF)
    key = -_fkey(l[ids]) if "zero_order" in mut else -l[ids].astype(np.float64)
    return ids[np.argsort(key, kind="stable")][:K]


def _ambig(a, b, eps):
    return (np.abs(a - b) <= eps * np.maximum(np.abs(a), np.abs(b))) if eps > 0 else np.zeros(np.shape(a), bool)


def chain(l, prm_row, seed, hl, eps=None, exact=False, mut=(), row=0, W=None, info=None):
    """Admissible tokens of one row of sample_topkp_kernel.  ``l``: the row after bias and penalties,
    ``hl``: the slot's ring length before the call (reset rows draw at position 0)."""
    p = parse(prm_row)
    eps = 0.0 if exact else (EPS if eps is None else eps)
    l = np.asarray(l, F32)
    od = order(l, k_of(p["temp"], p["top_k"], len(l), mut), mut)
    if len(od) == 0:
        return {0}
    if p["temp"] <= 0 or len(od) == 1:
        return {int(od[0])}
    pos = 0 if p["reset"] else int(hl)
    if "pos_mod_w" in mut:
        pos %= W
    uf = float(uniform(sample_hash(seed, p["rseed"], pos, row, mut))[0])
    v = l[od].astype(np.float64)
    e = np.exp((v - v[0]) / float(p["temp"]))
    incl = np.cumsum(e)
    if "drop_wave1" in mut and len(e) > 128:
        incl[128:] -= e[64:128].sum()
    before, lim = incl - e, float(p["top_p"]) * incl[-1]
    if exact:
        lim = float(F32(lim))
    yes = (before < lim) if "topp_lt" in mut else (before <= lim)
    amb = _ambig(before, lim, eps)
    sure, maybe = yes & ~amb, yes | amb
    if p["min_p"] > 0:
        mp = float(p["min_p"])
        amb = _ambig(e, mp, eps)
        sure, maybe = sure & (e >= mp) & ~amb, maybe & ((e >= mp) | amb)
    sure[0] = maybe[0] = True  # candidate 0: nothing before it, and min-p never drops it
    # the kernel keeps up to the LAST candidate that passes: every doubtful one past the sure ones may be it
    n_sure = int(np.flatnonzero(sure)[-1]) + 1
    nkeeps = {n_sure} | {int(j) + 1 for j in np.flatnonzero(maybe) if j + 1 > n_sure}
    toks = set()
    for nk in nkeeps:
        u = uf * incl[nk - 1]
        if exact:
            u = float(F32(u))
        c = incl[:nk]
        a3 = _ambig(c, u, eps)
        hit = np.flatnonzero(((c >= u) if "pick_ge" in mut else (c > u)) & ~a3)
        f = int(hit[0]) if len(hit) else nk - 1
        toks |= {int(od[f])} | {int(od[i]) for i in np.flatnonzero(a3[:f])}
    if info is not None:
        info.update(order=od, nkeeps=sorted(nkeeps), u01=uf)
    return toks


def _scores(l, temp, seed, row, step, allowed, cap):
    l = np.asarray(l, F32)
    ids = np.arange(len(l)) if allowed is None else np.unique(np.asarray(allowed))
    x = l[ids].astype(np.float64)
    if temp > 0:
        u = uniform(gumbel_hash(seed, row, step, ids), cap).astype(np.float64)
        with np.errstate(divide="ignore"):
            x = x / float(F32(temp)) - np.log(-np.log(u))
    return ids, x


def gumbel(l, temp, seed, row, step, allowed=None, eps_g=None, cap=True):
    """Admissible tokens of one row of select_kernel (``allowed``: the ids of a grammar row)."""
    eps_g = EPS_G if eps_g is None else eps_g
    ids, x = _scores(l, temp, seed, row, step, allowed, cap)
    best = x.max()
    if best == NINF:
        return {int(ids[0])}
    if temp <= 0 or best == np.inf:  # (+inf: the noise of u == 1 before the cap)
        return {int(ids[np.flatnonzero(x == best)[0]])}
    return {int(i) for i in ids[x >= best - 2 * eps_g * max(1.0, abs(best))]}


def gumbel_gap(l, temp, seed, row, step, tok, allowed=None):
    """How far the float64 score of ``tok`` lies below the row's best, relative to max(1, |best|): 0 for
    the model's own id, at most 2 * EPS_G for an admissible one."""
    ids, x = _scores(l, temp, seed, row, step, allowed, True)
    return float((x.max() - x[ids == tok][0]) / max(1.0, abs(x.max()))) if temp > 0 else 0.0


def needed_eps(tok, l, prm_row, seed, hl, **kw):
    """The smallest eps of 0, EPS / 64, EPS / 32, ..., EPS at which ``tok`` is admissible (inf: none):
    0 says that the kernel decided every comparison of the row as float64 does."""
    for eps in (0.0, *(EPS / 2 ** k for k in range(6, -1, -1))):
        if tok in chain(l, prm_row, seed, hl, eps=eps, **kw):
            return eps
    return float("inf")


def needs_radix(l, K):
    """Whether sample_topkp_kernel's candidate list overflows on this row (more than kCand entries at
    or above the K-th largest of the 1024 per-thread maxima), i.e. whether it takes the radix select."""
    l = np.asarray(l, F32)
    pad = np.full(-len(l) % THREADS, NINF, F32)
    tmax = np.concatenate([l, pad]).reshape(-1, THREADS).max(0)
    t0 = np.sort(tmax)[::-1][K - 1]
    return int(np.count_nonzero((l >= t0) & (l > NINF))) > KCAND


# ------------------------------------------------------------------------------------ float32 emulation
def scan32(e):
    """block_scan of csrc/sampling.hip on 1024 float32 values: a 64-lane shuffle scan per wave, then
    the serial sum of the earlier waves' totals."""
    v = np.asarray(e, F32).reshape(16, 64).copy()
    for o in (1, 2, 4, 8, 16, 32):
        t = np.zeros_like(v)
        t[:, o:] = v[:, :-o]
        v = v + t
    add, acc = np.zeros(16, F32), F32(0)
    for w in range(16):
        add[w] = acc
        acc = F32(acc + v[w, 63])
    return (v + add[:, None]).reshape(-1)


def measure_eps(l, prm_row):
    """Worst relative error of the float32 quantities the kernel compares on one row -- e (where
    e >= E_FLOOR), the mass before a candidate, the inclusive prefix -- against float64, plus 2^-24
    for the one further rounding of top_p * total and of u * kept."""
    p = parse(prm_row)
    od = order(l, k_of(p["temp"], p["top_k"], len(l)))
    v32 = np.asarray(l, F32)[od]
    x = (v32 - v32[0]) * (F32(1) / p["temp"])
    e32 = np.zeros(THREADS, F32)
    e32[:len(od)] = np.exp(x.astype(np.float64)).astype(F32)
    i32 = scan32(e32)[:len(od)]
    e32 = e32[:len(od)]
    e = np.exp((v32.astype(np.float64) - float(v32[0])) / float(p["temp"]))
    incl = np.cumsum(e)
    worst = np.max(np.abs(i32 - incl) / incl)
    big = e >= E_FLOOR
    worst = max(worst, np.max(np.abs(e32[big] - e[big]) / e[big]))
    if len(od) > 1:
        worst = max(worst, np.max(np.abs((i32 - e32)[1:] - incl[:-1]) / incl[:-1]))
    return float(worst) + 2.0 ** -24


def measure_eps_g(l, temp, seed, row, step):
    """Worst error of the float32 Gumbel score x * (1 / T) - log(-log u), every operation rounded,
    against float64, relative to max(1, |score|)."""
    l = np.asarray(l, F32)
    u = uniform(gumbel_hash(seed, row, step, np.arange(len(l))))
    inner = (-np.log(u.astype(np.float64))).astype(F32)
    g = (-np.log(inner.astype(np.float64))).astype(F32)
    s32 = l * (F32(1) / F32(temp)) + g
    s64 = l.astype(np.float64) / float(F32(temp)) - np.log(-np.log(u.astype(np.float64)))
    ok = np.isfinite(s64)
    return float(np.max(np.abs(s32[ok] - s64[ok]) / np.maximum(1.0, np.abs(s64[ok]))))


# ------------------------------------------------------------------------------------ inputs
RANDOM_PARAMS = ((0.8, 40, 0.9, 0.0), (1.0, 0, 1.0, 0.3), (0.5, 1000, 0.5, 0.0), (1.3, 64, 0.95, 0.05))
RANDOM_SPREADS = (2.0, 6.0)
RANDOM_V = (1025, 4096)
RANDOM_B = 256
RANDOM_SEED = 0x5DEECE66D  # above 2^32: the fold is part of every expected token


@functools.lru_cache(maxsize=None)
def random_logits(spread, V):
    rng = np.random.default_rng(int(spread * 1000) + V)
    return (rng.standard_normal((RANDOM_B, V)) * spread).astype(F32)


def random_cases():
    """(name, logits [256, V], prm [256, 8 or 12], hl [256]) of the random rows with margin."""
    out = []
    for spread in RANDOM_SPREADS:
        for V in RANDOM_V:
            for T, k, tp, mp in RANDOM_PARAMS:
                prm = prm_rows(RANDOM_B, 12 if mp > 0 else 8, T, k, tp, mp, seeds=np.arange(RANDOM_B) * 7919 - 1000)
                hl = np.arange(RANDOM_B) % 5
                out.append((f"randn*{spread:g} V{V} T{T} k{k} p{tp} m{mp}", random_logits(spread, V), prm, hl))
    return out


def unpinned_cap(prm_row, V):
    p = parse(prm_row)
    return 0.02 if k_of(p["temp"], p["top_k"], V) <= 64 else 0.10


GUMBEL_V = (1, 7, 8, 2043, 2048, 2056)
GUMBEL_TEMPS = (0.0, 0.5, 1.0, 2.0)
GUMBEL_SEEDS = (0x1234567890, (1 << 62) + 12345)
GUMBEL_STEPS = (0, 1, 4)
GUMBEL_B = 32


@functools.lru_cache(maxsize=None)
def gumbel_logits(V):
    """[32, V] values on the bf16 grid (the bf16 and the f32 kernels then read the same numbers)."""
    rng = np.random.default_rng(V)
    x = (rng.standard_normal((GUMBEL_B, V)) * 2).astype(F32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def gumbel_temps():
    return np.asarray([GUMBEL_TEMPS[(r * 7 // 3) % 4] for r in range(GUMBEL_B)], F32)


def plateau_logits(V, ids, value=1.0, below=-2.0):
    l = np.full(V, below, F32)
    l[np.asarray(ids)] = value
    return l


def radix_rows():
    """name -> (row [8192], top_k, exact): plateaus of more than kCand entries (needs_radix holds)."""
    V = 8192
    i = np.arange(V)
    rows = {}
    third = plateau_logits(V, i[(i >= 4096) | ((i % 3 == 0) & (i >= 60))])
    rows["ties on every third id, collected over four chunks"] = (third, 1024, True)
    above = plateau_logits(V, i[i >= 3000])
    above[[7, 2999, 3001, 5000, 8191]] = [1.5, 2.0, 1.25, 2.0, 1.75]
    rows["entries above the plateau, then ties"] = (above, 40, False)
    lo = np.full(V, -2.0, F32)
    lo[2000:] = (np.float32(1.0).view(np.uint32) + ((i[2000:] * 5) % 8).astype(np.uint32)).view(F32)
    rows["adjacent floats: the K-th key falls in digit 3"] = (lo, 1024, False)
    mid = np.full(V, -2.0, F32)
    mid[2000:] = (np.float32(1.0).view(np.uint32) + (((i[2000:] * 5) % 8).astype(np.uint32) << np.uint32(10))).view(F32)
    rows["middle digit: the K-th key falls in digit 2"] = (mid, 1024, False)
    rows["negative plateau"] = (plateau_logits(V, i[(i % 8 != 3) & (i > 100)], -1.5, -3.0), 40, True)
    rows["negative plateau, K 1024"] = (plateau_logits(V, i[(i % 8 != 3) & (i > 100)], -1.5, -3.0), 1024, True)
    masked = plateau_logits(V, i[(i % 5 != 0) & (i >= 1500)], 0.75, NINF)
    masked[[3, 1400]] = -1.0
    rows["masked entries around the plateau"] = (masked, 1024, True)
    zeros = plateau_logits(V, i[i >= 2000], 0.0, -1.0)
    zeros[(i >= 2000) & (i % 2 == 0)] = -0.0
    rows["plateau of zeros of both signs"] = (zeros, 40, True)
    return rows


# ------------------------------------------------------------------------------------ sampler cases
class Case:
    """One call of ops.sample: logits [B, V], prm [B, 8 | 12], the ring (hist [slots, W], filled with -1
    unless given, and its lengths hl [slots]) and the engine seed.  ``exact``: every kept value of every
    row is equal, so the expected token is a single one with no tolerance."""

    def __init__(self, name, logits, prm, hl=None, W=64, seed=123, exact=True, hist=None):
        self.name, self.logits, self.prm, self.W, self.seed, self.exact = name, np.asarray(logits, F32), prm, W, seed, exact
        slots = int(prm[:, 5].max()) + 1
        self.hl = np.zeros(slots, np.int32) if hl is None else np.asarray(hl, np.int32)
        self.hist = np.full((slots, W), -1, np.int32) if hist is None else np.asarray(hist, np.int32)

    def edited(self, r):
        """Row r after the repeat penalty over its window (the other edits are not used here)."""
        p = parse(self.prm[r])
        hl = 0 if p["reset"] else int(self.hl[p["slot"]])
        if p["pen"] == 1 or p["last_n"] == 0:
            return self.logits[r]
        return penalize(self.logits[r], p["pen"], window(self.hist[p["slot"]], hl, p["last_n"], self.W))

    def expected(self, mut=(), rows=None):
        """The admissible set of every row (or of ``rows``)."""
        return [chain(self.edited(r), self.prm[r], self.seed, int(self.hl[int(self.prm[r, 5])]), exact=self.exact,
                      mut=mut, row=r, W=self.W) for r in (range(len(self.prm)) if rows is None else rows)]

    def needed_eps(self, got):
        """The largest needed_eps over the rows for the tokens ``got``."""
        return max(needed_eps(int(got[r]), self.edited(r), self.prm[r], self.seed, int(self.hl[int(self.prm[r, 5])]), row=r,
                              W=self.W) for r in range(len(self.prm)))

    def position(self, r):
        return 0 if self.prm[r, 6] else int(self.hl[int(self.prm[r, 5])])


PLATEAU_K = (2, 8, 40, 1024)
PLATEAU_TEMPS = (0.5, 1.0)
PLATEAU_TOP_P = (0.0, 0.25, 0.5, 1.0, 1.5)


def _plateau_row(V=2600):
    return plateau_logits(V, np.arange(1, V, 2))  # 1300 ties on the odd ids


def _special_seeds(prm, hl, seed=123):
    """Rows 0..: the committed tuples of ``seed`` -- an integer u * 1024 and u01 == 1 before the cap."""
    r = 0
    for s, rseed, pos in INT_U_1024 + U1_SAMPLE:
        if s == seed:
            prm[r, 7], hl[prm[r, 5]] = rseed, pos
            prm[r].view(F32)[0:2] = 1.0, 1.0
            r += 1
    return r


@functools.lru_cache(maxsize=None)
def plateau_case(K, width):
    """256 rows of one 1300-wide plateau, top_k = K, every (temperature, top_p) of the lists over
    distinct request seeds and positions 0..3; kept count floor(top_p * K) + 1 clamped to K."""
    B = 256
    r = np.arange(B)
    prm = prm_rows(B, width, np.take(PLATEAU_TEMPS, r % 2), K, np.take(PLATEAU_TOP_P, (r // 2) % 5),
                   seeds=r * 2654435761 % (1 << 31) - (1 << 30))
    hl = (r % 4).astype(np.int32)
    _special_seeds(prm, hl)
    return Case(f"plateau K{K} w{width}", np.tile(_plateau_row(), (B, 1)), prm, hl)


@functools.lru_cache(maxsize=None)
def underflow_case(width):
    """300 candidates at v0 and 724 at v0 - 200 (e exactly 0 in float32): top_p = 1 keeps all of them
    and never picks the lower level -- not even with the draw that was u == 1.  12-wide rows add a tiny
    min_p, which drops the e = 0 entries and changes no pick."""
    B, V = 64, 2048
    row = plateau_logits(V, np.arange(1, 600, 2), 3.0, -197.0)
    prm = prm_rows(B, width, 1.0, 0, 1.0, 1e-30 if width == 12 else 0.0, seeds=np.arange(B) * 977 + 5)
    hl = (np.arange(B) % 4).astype(np.int32)
    _special_seeds(prm, hl)
    return Case(f"underflow w{width}", np.tile(row, (B, 1)), prm, hl)


@functools.lru_cache(maxsize=None)
def min_p_case():
    """min_p = 1 keeps every tie (e = 1 >= 1); the next float above 1 keeps candidate 0 alone."""
    B = 64
    mp = np.where(np.arange(B) % 2 == 0, F32(1.0), np.nextafter(F32(1.0), F32(2.0)))
    prm = prm_rows(B, 12, 1.0, np.take((8, 40, 1024, 0), np.arange(B) // 2 % 4), 1.0, mp, seeds=np.arange(B) * 31 + 1)
    return Case("min_p at 1 and above", np.tile(_plateau_row(), (B, 1)), prm)


SIZES_V = (1, 2, 40, 1023, 1024, 1025, 4097)


@functools.lru_cache(maxsize=None)
def sizes_case(V):
    """One value on the whole row (the candidates are ids 0..K-1) for top_k in {0, 1, V, V + 1, 5000}."""
    ks = (0, 1, V, V + 1, 5000)
    B = 8 * len(ks)
    prm = prm_rows(B, 8, 1.0, np.repeat(ks, 8), 1.0, seeds=np.arange(B) * 613 + V)
    return Case(f"sizes V{V}", np.full((B, V), -0.75 if V % 2 else 0.5, F32), prm)


PLACE_TUPLE = dict(rseed=424242, hl=5)


@functools.lru_cache(maxsize=None)
def placement_cases():
    """The same (logits, seed, request seed, position) at batch row 0 of 1 in slot 0 and at row 37 of
    64 in slot 9; sampled over a K = 1024 plateau, so a draw keyed on the row or the slot shows."""
    one = Case("placement B1", _plateau_row()[None], prm_rows(1, 8, 1.0, 0, 1.0, seeds=PLACE_TUPLE["rseed"]),
               [PLACE_TUPLE["hl"]])
    B = 64
    prm = prm_rows(B, 8, 1.0, 0, 1.0, slots=(np.arange(B) + 36) % B, seeds=np.arange(B) + 1000)
    prm[37, 7] = PLACE_TUPLE["rseed"]
    assert prm[37, 5] == 9
    hl = np.arange(B, dtype=np.int32) % 3
    hl[9] = PLACE_TUPLE["hl"]
    return one, Case("placement B64", np.tile(_plateau_row(), (B, 1)), prm, hl)


POS_W = 16
POS_HL = (0, 1, POS_W - 1, POS_W, 3 * POS_W + 5)


@functools.lru_cache(maxsize=None)
def position_case():
    """Ring lengths around W: the draw is keyed on the length itself, the append lands at length % W;
    the last row restarts its sequence (reset = 1) from a ring of length 7 and draws at position 0.
    Every row has the same request seed, so equal positions would give equal tokens."""
    B = len(POS_HL) + 1
    prm = prm_rows(B, 8, 1.0, 0, 1.0, seeds=77)
    prm[-1, 6] = 1
    return Case("position", np.tile(_plateau_row(), (B, 1)), prm, list(POS_HL) + [7], W=POS_W)


@functools.lru_cache(maxsize=None)
def zeros_case():
    """The row maximum is -0.0 at id 0 and +0.0 at id 5: they are equal, so id 0 comes first -- for the
    greedy rows, and as candidate 0 of the sampled ones (top_k = 2)."""
    B = 64
    row = np.full(8, -5.0, F32)
    row[0], row[5] = -0.0, 0.0
    prm = prm_rows(B, 8, np.where(np.arange(B) < 8, 0.0, 1.0), 2, 1.0, seeds=np.arange(B) * 101 + 9)
    return Case("zeros", np.tile(row, (B, 1)), prm)


@functools.lru_cache(maxsize=None)
def radix_case(name):
    row, k, exact = radix_rows()[name]
    B = 32
    # (top_p * K is no integer on the near-plateaus: there every row of a cut at one would be unpinned)
    prm = prm_rows(B, 8, 1.0, k, np.where(np.arange(B) % 4 == 3, 0.5 if exact else 0.7, 1.0), seeds=np.arange(B) * 7877 + 3)
    return Case(name, np.tile(row, (B, 1)), prm, exact=exact)


@functools.lru_cache(maxsize=None)
def random_case(i):
    name, logits, prm, hl = random_cases()[i]
    return Case(name, logits, prm, hl, seed=RANDOM_SEED, exact=False)


@functools.lru_cache(maxsize=None)
def penalty_case():
    """Random rows whose ring holds the row's own eight largest ids under a repeat penalty of 1.3: the
    draw follows the edited logits (the order of the candidates changes)."""
    logits = random_logits(2.0, 4096)
    T, k, tp, _ = RANDOM_PARAMS[0]
    prm = prm_rows(RANDOM_B, 8, T, k, tp, pen=1.3, last_n=6, seeds=np.arange(RANDOM_B) * 13 + 2)
    hist = np.full((RANDOM_B, 64), -1, np.int32)
    hist[:, :8] = np.argsort(-logits, axis=1, kind="stable")[:, :8]
    return Case("ring + repeat penalty", logits, prm, np.full(RANDOM_B, 8, np.int32), seed=RANDOM_SEED, exact=False,
                hist=hist)


def exact_cases():
    """Every case whose expected token carries no tolerance (what the mutants are run against)."""
    out = [plateau_case(K, w) for K in PLATEAU_K for w in (8, 12)]
    out += [underflow_case(8), underflow_case(12), min_p_case(), position_case(), zeros_case(), *placement_cases()]
    out += [sizes_case(V) for V in SIZES_V]
    return out + [radix_case(n) for n, (_, _, exact) in radix_rows().items() if exact]


# ------------------------------------------------------------------------------------ Gumbel cases
def allowed_plan(B, V, seed=0):
    """A select_allowed plan [B flags | B+1 offsets | ids] with every third row unconstrained, and the
    allowed ids of each row (None: the whole vocabulary)."""
    rng = np.random.default_rng(seed + V)
    rows = [None if r % 3 == 0 else np.sort(rng.choice(V, size=min(V, 1 + (r * 37) % 300), replace=False)) for r in range(B)]
    flags = np.asarray([0 if a is None else 1 for a in rows], np.int32)
    offs = np.concatenate([[0], np.cumsum([0 if a is None else len(a) for a in rows])]).astype(np.int32)
    ids = np.concatenate([a for a in rows if a is not None] or [np.zeros(0)]).astype(np.int32)
    return np.concatenate([flags, offs, ids]), rows
