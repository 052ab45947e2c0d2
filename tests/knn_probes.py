"""Structured cosine-kNN inputs whose answer pins every (query, row) score, every tie and every tile
edge of both routes of ``knn_topk`` (GEMM scores + chunked top-k, and the fused MFMA kernel), the
model that says which bits must come back, and the derived bound of the random tier.

The arithmetic the model pins (csrc/knn.hip: ``score = dot / (qn * cn + 1e-9f)``):

dot          operands are small integers that are exact in bf16 and |sum| < 2^24 (asserted), so every
             product and every partial sum is exact in f32 in ANY order: the MFMA accumulators of both
             routes, the LDS-DMA GEMM and the permuted k-order of the fused kernel must EQUAL the
             integer answer.
denominator  the kernels are built with -ffp-contract=fast: ``qn * cn + 1e-9f`` may be one FMA or two
             roundings.  Every probe uses norms whose product is exact in f32 (or overflows in both
             forms; asserted), so both agree: ``f32(f32(qn * cn) + f32(1e-9))``.
quotient     the correctly rounded f32 division (the compiler's default for HIP); no other value is
             admitted.
order        score descending, ties by ascending id, -0.0 == +0.0 is a tie, a NaN score is absent
             (never returned), (-inf, -1) pads, every one of the nq x K slots written.

There is no tolerance in the exact tier: returned scores are compared as bit patterns.

A top-K shows at most 64 rows per query.  To make every (query, row) pair count, ``rotation`` moves a
window of <= 64 rows over the corpus by way of the norms: cn = 1 inside, 2^40 outside, qn = 1 (eps is
absorbed in both denominators, so every score is an exact power-of-two scaling of an integer).
Window rows with a positive dot outrank everything else and, with K = 64, all come back; a second
launch with the negated queries returns the others.  ``observed`` is the account of it.

Families: S "dense sign" (+-1 operands, one coordinate of every row zeroed so each dot is odd: a
dropped, doubled or mispaired product moves a dot by >= 1), H "one-hot k" (row n holds one +1 / +2 at
k0(n) = (7 (n + off) + 3) % D, query j the asymmetric pattern (37 j + 11 k) % 251 - 125, so the score
names the k, the row and the query that were mixed up), the epilogue probes, the tie plateaus, the
NaN probes, and ``merge_case`` / ``merge_model`` for ``knn_merge`` alone.

Plain torch; the GPU test imports this module as a sibling.
"""
import functools
from typing import NamedTuple, Optional

import torch

import gemm_probes as G

BF = torch.bfloat16
F32 = torch.float32
EPS32 = torch.tensor(1e-9, dtype=F32)  # the kernels' 1e-9f
FAR = 2.0 ** 40  # cn of the rows outside the window
WIN = 64  # rows per window = the largest K
ROWS, QT, BN, SCH = 256, 32, 128, 4096  # fused block, fused query tile, GEMM column tile, top-k chunk
U = 2.0 ** -24
NEG_INF = float("-inf")


class Launch(NamedTuple):
    what: str
    c: torch.Tensor  # [N, D] bf16
    cn: torch.Tensor  # [N] f32
    q: torch.Tensor  # [nq, D] bf16
    qn: torch.Tensor  # [nq] f32
    K: int
    dot: torch.Tensor  # [nq, N] f64, the exact answer of q c^T
    k0: Optional[torch.Tensor] = None  # H: the hot k of every row


# --- the model ----------------------------------------------------------------------------------
def f32_toward_zero(x):
    """float64 -> f32, rounded toward zero."""
    f = x.float()
    over = f.double().abs() > x.abs()
    return torch.where(over, torch.nextafter(f, torch.zeros_like(f)), f)


def denominators(cn, qn, eps=True):
    """f32 [nq, N]: f32(f32(qn * cn) + f32(1e-9)); asserts the product is exact (or overflows)."""
    prod = qn.float()[:, None] * cn.float()[None, :]
    exact = prod.double() == qn.double()[:, None] * cn.double()[None, :]
    assert bool((exact | torch.isinf(prod)).all()), "qn * cn is not exact in f32: FMA and two roundings differ"
    return prod + EPS32 if eps else prod


def model_scores(dot, cn, qn, eps="in", div="rne"):
    """f32 [nq, N] scores of an exact f64 ``dot``.  eps in / none / outside and div rne / trunc are the
    kernels' epilogue and its mutants."""
    fin = dot[torch.isfinite(dot)]
    assert fin.numel() == 0 or float(fin.abs().max()) < 2 ** 24, "|dot| >= 2^24: not exact in every order"
    d32 = dot.float() + 0.0  # (accumulators start at +0.0: an exact zero dot is +0.0)
    den = denominators(cn, qn, eps == "in")
    if div == "trunc":
        s = f32_toward_zero(d32.double() / den.double())
    else:
        s = d32 / den
    return s + EPS32 if eps == "outside" else s


def topk_model(score, K, ties="asc", skip_kth=False):
    """(scores f32 [nq, K], ids int32 [nq, K]) of f32 [nq, N] scores: descending, ties by ascending id,
    -0.0 == +0.0, NaN absent, (-inf, -1) pads.  ``ties='desc'`` and ``skip_kth`` are mutants."""
    nq, N = score.shape
    out_s = torch.full((nq, K), NEG_INF, dtype=F32)
    out_i = torch.full((nq, K), -1, dtype=torch.int32)
    if N == 0 or nq == 0:
        return out_s, out_i
    valid = ~torch.isnan(score)
    key = torch.where(valid, -score + 0.0, torch.full_like(score, float("inf")))
    if ties == "desc":
        order = (N - 1) - torch.sort(key.flip(1), dim=1, stable=True).indices
    else:
        order = torch.sort(key, dim=1, stable=True).indices
    if skip_kth and N > K:
        order = torch.cat([order[:, : K - 1], order[:, K:]], dim=1)
    kk = min(K, N)
    order = order[:, :kk]
    ok = torch.arange(kk)[None, :] < valid.sum(1, keepdim=True)
    out_s[:, :kk] = torch.where(ok, score.gather(1, order), out_s[:, :kk])
    out_i[:, :kk] = torch.where(ok, order.int(), out_i[:, :kk])
    return out_s, out_i


MUTANTS = ("drop_row", "skip_chunk", "swap_lr4", "swap_qcol", "no_eps", "eps_outside", "trunc_div",
           "ties_desc", "skip_kth", "unclamped")


def model(L, mutant=None):
    """What ``knn_topk`` must return for a Launch; ``mutant`` names one of the subtly wrong kernels."""
    dot, cn, qn = L.dot, L.cn, L.qn
    nq, N = dot.shape
    if mutant == "skip_chunk" and N:  # the 8 elements of k-step u = 2 of group g = 1, half h = 1
        sl = slice(64 * 1 + 32 * 1 + 8 * 2, 64 * 1 + 32 * 1 + 8 * 2 + 8)
        dot = dot - L.q[:, sl].double() @ L.c[:, sl].double().t()
    s = model_scores(dot, cn, qn, eps={"no_eps": "none", "eps_outside": "outside"}.get(mutant, "in"),
                     div="trunc" if mutant == "trunc_div" else "rne")
    if mutant == "drop_row" and N > ROWS + 37:  # one row of the second 256-block
        s[:, ROWS + 37] = float("nan")
    if mutant == "swap_lr4" and N:  # rows lr and lr ^ 4 of the C layout
        n = torch.arange(N)
        p = torch.where((n ^ 4) < N, n ^ 4, n)
        p = torch.where(p[p] == n, p, n)
        s = s[:, p]
    if mutant == "swap_qcol" and nq > QT:  # query columns r and r ^ 1 of the second query tile
        pad = torch.zeros(2 * QT - nq, N, dtype=F32) if nq < 2 * QT else s[:0]
        full = torch.cat([s, pad])  # (a column past nq holds a zero query)
        j = torch.arange(full.shape[0])
        full = full[torch.where((j >= QT) & (j < 2 * QT), QT + ((j - QT) ^ 1), j)]
        s = full[:nq]
    if mutant == "unclamped" and N:  # row n_rows (the clamped load's copy of the last row) scored as valid
        s = torch.cat([s, model_scores(dot[:, N - 1:], torch.ones(1), qn)], dim=1)
    return topk_model(s, L.K, ties="desc" if mutant == "ties_desc" else "asc", skip_kth=mutant == "skip_kth")


def bits(s):
    return s.contiguous().view(torch.int32)


def same(a, b):
    """Two (scores, ids) results are the same bits."""
    return bool(torch.equal(bits(a[0].cpu()), bits(b[0].cpu())) and torch.equal(a[1].cpu(), b[1].cpu()))


def check_exact(s, i, L, route=""):
    """The returned (s, i) equal the model bit for bit; the failure names the first wrong slot."""
    ws, wi = model(L)
    s, i = s.cpu(), i.cpu()
    assert s.shape == ws.shape and i.shape == wi.shape and s.dtype == F32 and i.dtype == torch.int32, \
        f"{route} {L.what}: shapes {tuple(s.shape)} {tuple(i.shape)}, want {tuple(ws.shape)}"
    bad = (bits(s) != bits(ws)) | (i != wi)
    if not bool(bad.any()):
        return
    j, p = (int(v) for v in bad.nonzero()[0])
    gi, wid = int(i[j, p]), int(wi[j, p])
    msg = (f"{route} {L.what}: N={L.c.shape[0]} D={L.c.shape[1]} nq={L.q.shape[0]} K={L.K}: {int(bad.sum())} of "
           f"{bad.numel()} slots off; the first at query {j} (query tile {j // QT}, column {j % QT}), position {p}: "
           f"got (score {float(s[j, p])!r}, id {gi}), want ({float(ws[j, p])!r}, {wid})")
    for name, n in (("got", gi), ("wanted", wid)):
        if 0 <= n < L.c.shape[0]:
            msg += (f"; the {name} row {n} (256-block {n // ROWS} row {n % ROWS}, 128-tile {n // BN}, chunk {n // SCH}) "
                    f"has dot {float(L.dot[j, n])!r}, cn {float(L.cn[n])!r}")
            if L.k0 is not None:
                msg += f", k0 {int(L.k0[n])}"
    raise AssertionError(msg)


def observed(i, N):
    """bool [nq, N]: the (query, row) pairs whose id is in the returned list."""
    i = i.cpu().long()
    seen = torch.zeros(i.shape[0], N + 1, dtype=torch.bool)
    seen.scatter_(1, torch.where(i >= 0, i, torch.full_like(i, N)), True)
    return seen[:, :N]


# --- builders -----------------------------------------------------------------------------------
def _bf16_exact(t, what):
    return G._exact(t, what)


def sign_case(N, D, nq, seed=0):
    """S: +-1 queries, +-1 corpus with c[n, n % D] = 0 (D even: every dot is odd).  -> c, q, dot."""
    q, c = G.dense_sign(nq, N, D, seed=seed)
    c = c.clone()
    n = torch.arange(N)
    c[n, n % D] = 0
    dot = G.expect(q, c)
    assert D % 2 == 0 and bool((dot % 2 != 0).all()) and float(dot.abs().max()) < 2 ** 24
    return _bf16_exact(c.float(), "corpus"), q, dot


def hot_case(N, D, nq, off=0):
    """H -> c, q, dot, k0."""
    n = torch.arange(N)
    k0 = (7 * (n + off) + 3) % D
    c = torch.zeros(N, D)
    c[n, k0] = 1.0 + (n % 3 == 1).float()
    c, q = _bf16_exact(c, "one-hot"), G.pattern(nq, D)
    dot = q.double()[:, k0] * c.double()[n, k0][None, :]
    assert torch.equal(dot, G.expect(q, c)) and float(dot.abs().max()) < 2 ** 24
    return c, q, dot, k0


def hot_offsets(N, D):
    """Offsets after which k0 has walked all of D."""
    return list(range(0, D, N)) if N < D else [0]


def all_windows(N):
    return [(a, min(a + WIN, N)) for a in range(0, N, WIN)]


def edge_windows(N):
    """The first window, the last one, and the one centred on every tile, block and chunk edge below N
    that the nearest multiples of 128, 256 and 4096 give."""
    w = {(0, min(WIN, N)), (max(0, N - WIN), N)}
    for t in (BN, ROWS, SCH):
        for e in {t, (N - 1) // t * t}:
            if 0 < e < N:
                w.add((max(0, e - WIN // 2), min(N, e + WIN // 2)))
    return sorted(w)


def window_cn(N, a, b):
    cn = torch.full((N,), FAR, dtype=F32)
    cn[a:b] = 1.0
    return cn


def rotation(what, c, q, dot, windows, K=WIN, k0=None):
    """Two launches per window (q and -q) with cn = 1 inside the window, 2^40 outside."""
    N, nq = c.shape[0], q.shape[0]
    qn, neg = torch.ones(nq, dtype=F32), _bf16_exact(-q.float(), "-q")
    out = []
    for a, b in windows:
        assert b - a <= WIN
        cn = window_cn(N, a, b)
        out.append(Launch(f"{what} window [{a}, {b}) +q", c, cn, q, qn, K, dot, k0))
        out.append(Launch(f"{what} window [{a}, {b}) -q", c, cn, neg, qn, K, -dot, k0))
    return out


def coverage(kind, N, D, nq, windows=None, K=WIN):
    """-> (launches, must): the rotation of one family over ``windows`` (default: all of them), and
    the bool [nq, N] pairs that must be observed (all of the windows' rows; H: those with a non-zero
    dot -- the pattern holds a zero once in 251)."""
    windows = all_windows(N) if windows is None else windows
    rows = torch.zeros(N, dtype=torch.bool)
    for a, b in windows:
        rows[a:b] = True
    if kind == "S":
        c, q, dot = sign_case(N, D, nq, seed=nq)
        return rotation(f"S D={D}", c, q, dot, windows, K), rows[None, :].expand(nq, N).clone()
    out, must = [], torch.zeros(nq, N, dtype=torch.bool)
    for off in hot_offsets(N, D):
        c, q, dot, k0 = hot_case(N, D, nq, off)
        out += rotation(f"H D={D} off={off}", c, q, dot, windows, K, k0)
        must |= (dot != 0) & rows[None, :]
    assert float(must.double().mean()) >= 0.98 * float(rows.double().mean())
    return out, must


def epilogue(D=128, N=2 * ROWS + 37, nq=5, K=WIN):
    """The epilogue probes 3a-3e on S dots (odd integers)."""
    c, q, dot = sign_case(N, D, nq, seed=3)
    one, n = torch.ones(nq, dtype=F32), torch.arange(N)
    out = [Launch("3a qn = cn = 2^-15", c, torch.full((N,), 2.0 ** -15), q, torch.full((nq,), 2.0 ** -15), K, dot)]
    cn = torch.tensor([3.0, 5.0, 7.0, 11.0])[n % 4]
    out.append(Launch("3b denominators 3, 5, 7, 11", c, cn, q, one, K, dot))
    out.append(Launch("3b denominators 3, 5, 7, 11 at K = 10", c, cn.roll(1), q, one, 10, dot))
    cn = torch.where(n % 5 == 0, torch.zeros(N), torch.ones(N))
    out.append(Launch("3c cn = 0 with a non-zero dot", c, cn, q, one, K, dot))
    # 3d: two all-zero rows (one per 256-block) and an all-zero query, with their true norms 0
    cz, qz = c.clone(), q.clone()
    cz[[70, ROWS + 9]] = 0
    qz[2] = 0
    cn, qn = torch.full((N,), 8.0), torch.full((nq,), 8.0)
    cn[[70, ROWS + 9]] = 0
    qn[2] = 0
    out.append(Launch("3d zero row and zero query", cz, cn, qz, qn, K, G.expect(qz, cz)))
    # 3e: qn * cn = +inf for query 0 (and 2^100, 2^0 for the others): +-0.0 all tie, id order
    qn = torch.tensor([2.0 ** 100, 1.0, 2.0 ** -100, 2.0 ** 100, 1.0])[:nq]
    out.append(Launch("3e qn * cn = +inf", c, torch.full((N,), 2.0 ** 100), q, qn, K, dot))
    return out


def division_separates(L):
    """Some returned score of L differs between the correctly rounded and the truncating division."""
    return not same(model(L), model(L, "trunc_div"))


def ties(D=128, N=SCH + 131, K=WIN):
    """Plateaus of identical rows: A (81 rows, longer than K) straddles the 128-row tile edge, B the
    256-block edge, the 4096-chunk edge and two lone rows in other blocks, C (111 rows) ends at the last
    row.  The other rows are +-1 (no zeroed coordinate): their dots are even integers, so the lists
    below the plateaus are full of ties of their own.  Query j = the plateau's vector (j < 3), its
    negation (3) or a +-1 row."""
    q, c = G.dense_sign(6, N, D, seed=17)
    c, q = c.clone(), q.clone()
    rows = {0: list(range(100, 181)), 1: list(range(250, 262)) + list(range(SCH - 6, SCH + 6)) + [600, 1300],
            2: list(range(SCH + 20, N))}
    for j, r in rows.items():
        c[r] = q[j]
    q[3] = -q[0]
    dot, one = G.expect(q, c), torch.ones(6, dtype=F32)
    out = [Launch(f"ties K={k}", c, torch.ones(N, dtype=F32), q, one, k, dot) for k in (K, 10, 1)]
    # the same corpus cut inside plateau C: the tail block holds fewer than K rows
    M = SCH + 50
    out.append(Launch("ties, cut tail", c[:M], torch.ones(M, dtype=F32), q, one, K, dot[:, :M]))
    return out, rows


def nan_launches(D=128, N=ROWS + 44, nq=3, K=WIN):
    """One corpus row of NaN (absent from every list) and one query of NaN (a list of pads)."""
    c, q, dot = sign_case(N, D, nq, seed=5)
    c, q = c.clone(), q.clone()
    c[ROWS + 3, 77] = float("nan")
    q[1, 5] = float("nan")
    dot = dot.clone()
    dot[:, ROWS + 3] = float("nan")
    dot[1] = float("nan")
    cn = torch.ones(N, dtype=F32)
    cn[:WIN] = 4.0  # the first 64 rows pushed down, so K = 64 reaches past them and the NaN row's place shows
    return [Launch(f"NaN row and NaN query K={k}", c, cn, q, torch.ones(nq, dtype=F32), k, dot) for k in (K, 10)]


# --- knn_merge alone ------------------------------------------------------------------------------
def merge_model(cs, ci, K, keep_negative=False):
    """Candidates with id >= 0 and a non-NaN score, sorted by (-score, id); (-inf, -1) pads.  A
    (-inf, id >= 0) candidate is an ordinary one that ranks below every finite score."""
    nq = cs.shape[0]
    out_s = torch.full((nq, K), NEG_INF, dtype=F32)
    out_i = torch.full((nq, K), -1, dtype=torch.int32)
    for r in range(nq):
        p = [(-s + 0.0, i, s) for s, i in zip(cs[r].tolist(), ci[r].tolist()) if (i >= 0 or keep_negative) and s == s]
        p.sort(key=lambda t: t[:2])
        for j, (_, i, s) in enumerate(p[:K]):
            out_s[r, j], out_i[r, j] = s, i
    return out_s, out_i


ID_MAX = 2 ** 31 - 2


def merge_case(nq, ncand, seed=0):
    """-> (cs f32 [nq, ncand], ci int32): scores from 17 values (ties everywhere, -0.0 and +0.0 among
    them), distinct ids per query up to 2^31 - 2, every 7th id -1 (whatever its score), and planted:
    one score at candidates 3, 70, 259 and 999 (other waves and strides of the 256-thread loop), a
    (-inf, id >= 0), a NaN and a (+inf, -1) candidate."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * ncand + nq)
    cs = (torch.randint(-8, 9, (nq, ncand), generator=g).float() / 4)
    cs = torch.where(torch.rand(nq, ncand, generator=g) < 0.1, -cs * 0.0, cs)  # +-0.0
    ci = torch.empty(nq, ncand, dtype=torch.int64)
    for r in range(nq):
        ci[r] = (torch.randperm(4 * ncand + 8, generator=g)[:ncand] + 1) * (ID_MAX // (4 * ncand + 10))
    ci[:, 0] = ID_MAX
    if ncand > 1:
        ci[:, ncand - 1] = 0
    slot = torch.arange(ncand)[None, :] + torch.arange(nq)[:, None]
    ci = torch.where(slot % 7 == 5, torch.full_like(ci, -1), ci)
    for r in range(nq):
        for col in (3, 70, 259, 999):
            if col < ncand:
                cs[r, col] = 2.25
        if ncand >= 63:
            cs[r, 10], cs[r, 11], cs[r, 12] = NEG_INF, float("nan"), float("inf")
            ci[r, 10], ci[r, 11], ci[r, 12] = max(int(ci[r, 10]), 1), max(int(ci[r, 11]), 2), -1
    for r in range(nq):
        v = ci[r][ci[r] >= 0]
        assert v.unique().numel() == v.numel(), "ids of one query are distinct"
    return cs, ci.int()


# --- the random tier ------------------------------------------------------------------------------
RANDOM_SHAPES = [(777, 256), (3000, 128), (2000, 512), (1000, 768), (5000, 1024), (1300, 384)]
RANDOM_NQ, RANDOM_K, RANDOM_SEED = 40, 10, 11
UNPINNED_CAP = 0.05
# The cap is asserted from the float64 reference alone (tests/test_knn_probes_cpu.py).  B grows with D
# while the gaps between the best ten of a randn corpus shrink with 1 / sqrt(D): at D = 1024 (B about
# 4e-5) the reference's own unpinned share is 5.5 - 11.5 % for seeds 11..40 at N = 5000 and no smaller
# at N = 150..1100, so that shape uses the first later seed at which the reference meets the cap (3 %).
RANDOM_SEEDS = {(5000, 1024): 86}


@functools.lru_cache(maxsize=None)
def random_case(N, D, nq=RANDOM_NQ, K=RANDOM_K, seed=None):
    seed = RANDOM_SEEDS.get((N, D), RANDOM_SEED) if seed is None else seed
    return _random_case(N, D, nq, K, seed)


def _random_case(N, D, nq, K, seed):
    """randn bf16 corpus and queries with their f32 norms, the float64 scores, the derived bound

        B = gamma_D * sum_k |q_k c_k| / den + 3 u |s|,   gamma_D = D u / (1 - D u),  u = 2^-24

    (any summation order of the f32 dot, the denominator's two roundings and the division), the
    reference's first K + 1 ids per query, and which of the K positions are pinned: the float64 gaps
    to both neighbours exceed the sum of the two bounds."""
    g = torch.Generator().manual_seed(seed + 1000 * D + N)
    c = torch.randn(N, D, generator=g).to(BF)
    q = torch.randn(nq, D, generator=g).to(BF)
    cn, qn = c.double().norm(dim=1).float(), q.double().norm(dim=1).float()
    den = qn.double()[:, None] * cn.double()[None, :] + EPS32.double()
    s64 = (q.double() @ c.double().t()) / den
    gamma = D * U / (1 - D * U)
    B = gamma * (q.double().abs() @ c.double().abs().t()) / den + 3 * U * s64.abs()
    order = torch.sort(-s64, dim=1, stable=True).indices[:, : K + 1]
    rs, rb = s64.gather(1, order), B.gather(1, order)
    gap_ok = (rs[:, :-1] - rs[:, 1:]) > (rb[:, :-1] + rb[:, 1:])  # [nq, K]: position j against j + 1
    pinned = gap_ok.clone()
    pinned[:, 1:] &= gap_ok[:, :-1]
    return dict(c=c, q=q, cn=cn, qn=qn, s64=s64, B=B, order=order, pinned=pinned, K=K,
                unpinned=float((~pinned).double().mean()))


def check_random(s, i, r, what=""):
    """-> worst |score - fp64| / B.  Every returned score lies within B of the float64 score of the
    returned id; a pinned position holds the reference's id; at an unpinned one the id comes from the
    rows whose float64 score is within the bounds of the expected one; no id repeats."""
    s, i, K = s.cpu().double(), i.cpu().long(), r["K"]
    assert s.shape == (r["q"].shape[0], K) and bool((i >= 0).all()) and bool((i < r["c"].shape[0]).all()), what
    got64, gotB = r["s64"].gather(1, i), r["B"].gather(1, i)
    ratio = (s - got64).abs() / gotB
    assert float(ratio.max()) <= 1.0, f"{what}: a score is {float(ratio.max()):.3f} x its bound away from fp64"
    want = r["order"][:, :K]
    wrong = r["pinned"] & (i != want)
    assert not bool(wrong.any()), f"{what}: pinned position {tuple(wrong.nonzero()[0].tolist())} holds another id"
    near = (got64 - r["s64"].gather(1, want)).abs() <= gotB + r["B"].gather(1, want)
    assert bool(near.all()), f"{what}: an unpinned position holds a row outside the bounds"
    assert all(len(set(row)) == K for row in i.tolist()), f"{what}: an id repeats"
    return float(ratio.max())
