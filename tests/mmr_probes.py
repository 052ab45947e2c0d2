"""Shared inputs of the MMR tests (the fp32 reference on the CPU, csrc/mmr.hip on the GPU).

Exact probes, modelled in integer arithmetic.  Every corpus row has entries in {-1, 0, +1} and exactly
16 non-zeros, so its norm is 4 exactly, ``4 * 4 + 1e-9`` rounds to 16 in fp32 and every similarity is
an integer / 16.  ``rel`` is in sixteenths in [-1, 1] and ``lam`` in quarters, so every ``mmr_i = lam *
rel_i - (1 - lam) * m_i`` is a multiple of 1/64 whose two products and difference are exact in fp32
whatever the contraction: the expected outputs are computed in int64 sixty-fourths, picks by
``(-mmr, position)``, and compared bit for bit.

The one place where bits are not decided by the value is a zero: IEEE gives ``(-0) - (+0) = -0``, which
an ``mmr`` of value 0 is exactly when ``lam = 0`` and ``rel < 0`` (``lam * rel = -0``; the penalty ``1 *
m`` is ``+0``).  The model writes that sign; -0 and +0 compare equal, so the order is not affected.
"""
import numpy as np
import torch

N = 200
# planted rows (corpus()): ROW0 and its exact copies, its opposite (also the last row, id N - 1), and an
# orthogonal pair on ROW0's support
COPIES = (0, 1, 2, 3, 40, 41)
OPPOSITE = (50, N - 1)
ORTHO = (60, 61)
LAMS4 = (0, 1, 2, 3, 4)  # lam in quarters


def corpus(D, seed=0):
    """int8 [N, D]: 16 non-zeros (+-1) per row, drawn from a pool of <= 32 columns spread over the whole
    row (column 0 and D - 1 in it) so that rows overlap and their dots take many values."""
    rng = np.random.default_rng(1000 + D + seed)
    edges = (np.arange(33) * D) // 32
    pool = sorted({0, D - 1} | {int(rng.integers(lo, hi)) for lo, hi in zip(edges[:-1], edges[1:]) if hi > lo})
    pool = np.array(pool)
    assert len(pool) >= 16
    X = np.zeros((N, D), np.int8)
    for i in range(N):
        X[i, rng.choice(pool, 16, replace=False)] = rng.choice([-1, 1], 16)
    first = pool[:16]
    for i in COPIES[1:]:
        X[i] = X[0]
    for i in OPPOSITE:
        X[i] = -X[0]
    X[ORTHO[0]] = 0
    X[ORTHO[0], first] = 1
    X[ORTHO[1]] = 0
    X[ORTHO[1], first] = np.tile([1, -1], 8)
    assert np.all((X != 0).sum(1) == 16)
    return X


def mixed_row(C, rng):
    """One candidate row with every pattern that fits into C positions -> (ids, rel16, nan)."""
    ids = rng.integers(0, N, C).astype(np.int64)
    r16 = rng.integers(-16, 17, C).astype(np.int64)
    nan = np.zeros(C, bool)
    head = [0, 1, N - 1, ORTHO[0], ORTHO[1], 2, 50, 3]     # copies at 0 / 1, the opposite, the orthogonal pair
    ids[:min(C, len(head))] = head[:C]
    if C >= 2:
        r16[1] = r16[0] = 12                               # equal mmr in every round: position 0 before 1
    if C >= 6:
        ids[5] = ids[4]                                    # a duplicated id (two candidates)
    if C >= 8:
        r16[5] = r16[7] = 12                               # ... and more members of the tie group
    if C >= 33:
        ids[31], ids[32] = COPIES[4], COPIES[5]            # a tie across the 32 boundary
        r16[31] = r16[32] = 12
    if C >= 12:
        ids[C // 2 + 3] = -1                               # absent in the middle
        ids[C // 2 + 4] = N                                # the first id that is out of range
        ids[C // 2 + 5] = 2 ** 31 - 1
        nan[C // 3] = True                                 # a NaN rel
    if C >= 3:
        ids[C - 1] = -1                                    # a pad at the tail
    return ids, r16, nan


def make_case(D, C, K, nq, lam4, seed=0):
    """A probe batch: row q is `mixed` (q % 3 == 0), has max(K - 1, 1) present candidates scattered
    between pads (q % 3 == 1: fewer than K for K > 1) or has none (q % 3 == 2)."""
    rng = np.random.default_rng(7 + 131 * D + 17 * C + 5 * K + nq + seed)
    ids = np.empty((nq, C), np.int64)
    r16 = np.empty((nq, C), np.int64)
    nan = np.zeros((nq, C), bool)
    for q in range(nq):
        ids[q], r16[q], nan[q] = mixed_row(C, rng)
        if q % 3 == 1:
            keep = rng.choice(C, min(C, max(K - 1, 1)), replace=False)
            gone = np.ones(C, bool)
            gone[keep] = False
            ids[q, gone] = -1
            nan[q] = False
            ids[q, keep] = rng.choice([0, N - 1, 50, 7, 9], len(keep))
        elif q % 3 == 2:
            ids[q] = rng.choice([-1, N, N + 7, -5], C)
            ids[q, 0] = 3
            nan[q] = False
            nan[q, 0] = True                               # a valid id, absent through its NaN rel
    return dict(D=D, C=C, K=K, nq=nq, lam4=lam4, X=corpus(D, seed), ids=ids, r16=r16, nan=nan)


def probe_queries(X, nq):
    """int8 [nq, D] query vectors for a search over the probe corpus: corpus rows with the sign of their
    first three non-zeros flipped (16 non-zeros still, so every cosine is an integer / 16)."""
    Q = X[(7 * np.arange(nq)) % len(X)].copy()
    for q in Q:
        nz = np.flatnonzero(q)[:3]
        q[nz] = -q[nz]
    return Q


def model(X, ids, r16, nan, lam4, K):
    """The expected outputs in integers -> (pos, ids, rel, mmr, max_sim) as int32 / float32 arrays."""
    nq, C = ids.shape
    n = X.shape[0]
    o_pos = np.full((nq, K), -1, np.int32)
    o_id = np.full((nq, K), -1, np.int32)
    o_rel = np.full((nq, K), -np.inf, np.float32)
    o_mmr = np.full((nq, K), -np.inf, np.float32)
    o_sim = np.full((nq, K), -np.inf, np.float32)
    Xi = X.astype(np.int64)
    for q in range(nq):
        inside = (ids[q] >= 0) & (ids[q] < n)
        avail = inside & ~nan[q]
        rows = Xi[np.where(inside, ids[q], 0)]
        G = rows @ rows.T                                  # sim * 16
        m16 = np.zeros(C, np.int64)
        for r in range(K):
            v64 = lam4 * r16[q] - (4 - lam4) * m16
            cand = np.flatnonzero(avail)
            if not len(cand):
                break
            p = int(min(cand, key=lambda i: (-v64[i], i)))
            mmr = np.float32(v64[p] / 64.0)
            if v64[p] == 0 and lam4 == 0 and r16[q, p] < 0:
                mmr = np.float32(-0.0)                     # (-0) - (+0), see the module's docstring
            o_pos[q, r], o_id[q, r] = p, ids[q, p]
            o_rel[q, r], o_mmr[q, r], o_sim[q, r] = r16[q, p] / 16.0, mmr, m16[p] / 16.0
            avail[p] = False
            m16 = G[:, p].copy() if r == 0 else np.maximum(m16, G[:, p])
    return o_pos, o_id, o_rel, o_mmr, o_sim


def expected(case):
    return model(case["X"], case["ids"], case["r16"], case["nan"], case["lam4"], case["K"])


def tensors(case, device="cpu"):
    """(corpus bf16, cnorm f32, cand_id int32, rel f32, lam) of a case."""
    X = torch.from_numpy(case["X"].astype(np.float32)).to(torch.bfloat16)
    rel = case["r16"].astype(np.float32) / np.float32(16)
    rel[case["nan"]] = np.nan
    cn = torch.full((X.shape[0],), 4.0)
    cid = torch.from_numpy(case["ids"].astype(np.int32))
    return X.to(device), cn.to(device), cid.to(device), torch.from_numpy(rel).to(device), case["lam4"] / 4.0


def check_exact(out, case, what=""):
    names = ("pos", "ids", "rel", "mmr", "max_sim")
    for name, got, want in zip(names, out, expected(case)):
        got = got.cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape, (what, name, got.dtype, got.shape)
        same = got.view(np.int32) == want.view(np.int32)
        if not same.all():
            q, r = np.argwhere(~same)[0]
            raise AssertionError(f"{what} {name}[{q}, {r}]: got {got[q, r]!r}, expected {want[q, r]!r}; "
                                 f"row got {got[q].tolist()} expected {want[q].tolist()}")


SWEEP_D = (16, 48, 128, 768, 1024)
SWEEP_C = (1, 2, 31, 32, 33, 64)


def sweep():
    """(D, C, K, nq, lam4) of the issue's sweep, lam cycling through its five values."""
    n = 0
    for D in SWEEP_D:
        for C in SWEEP_C:
            for K in sorted({1, min(6, C), C}):
                for nq in (1, 3):
                    yield D, C, K, nq, LAMS4[n % 5]
                    n += 1


# ---------------------------------------------------------------- random rows: fp64 and the bound
U = 2.0 ** -24


def random_case(D, seed=0, n=1000, nq=33, planted=120):
    """Gaussian bf16 rows, `planted` of them near-copies (a row plus small noise) of other rows, and nq
    queries that are noisy copies of corpus rows (so their neighbourhoods hold the near-copies)."""
    g = torch.Generator().manual_seed(100 + D + seed)
    X = torch.randn(n, D, generator=g)
    src = torch.randint(0, n - planted, (planted,), generator=g)
    X[n - planted:] = X[src] + 0.05 * torch.randn(planted, D, generator=g)
    Q = X[torch.randint(0, n, (nq,), generator=g)] + 0.5 * torch.randn(nq, D, generator=g)
    return X.to(torch.bfloat16), Q.to(torch.bfloat16)


def sims_fp64(corpus, cnorm, ids):
    """fp64 similarities between the candidates of one row on the kernel's inputs -> [C, C]."""
    rows = corpus[ids.long()].double()
    cn = cnorm[ids.long()].double()
    return (rows @ rows.T) / (cn[:, None] * cn[None, :] + 1e-9)


def check_against_fp64(out, corpus, cnorm, cand_id, rel, lam, K, ref_ids=None):
    """Round by round, given the kernel's own earlier picks (docs/mmr.md, "The bound"): every reported
    max_sim within e_sim = (D + 4) 2^-24 of its fp64 value; every pick's fp64 mmr no lower than the
    fp64 best of its round minus 2 e_mmr, e_mmr = (1 - lam) e_sim + 3 * 2^-24 (lam |rel| + (1 - lam) |m|),
    taken at the larger of the pick's and the best's; and, with ``ref_ids``, the kernel's id equal to
    the fp32 reference's wherever the fp64 margin between the round's first and second exceeds 2 e_mmr.
    lam and 1 - lam enter the fp64 evaluation as the kernel gets them: lam as fp32, 1 - lam formed in
    fp32.  -> (worst |max_sim - fp64| / e_sim, worst shortfall / (2 e_mmr), rounds compared with ref)."""
    pos, ids, _, _, ms = (t.cpu() for t in out)
    corpus, cnorm, cand_id, rel = corpus.cpu(), cnorm.cpu(), cand_id.cpu(), rel.cpu()
    D = corpus.shape[1]
    e_sim = (D + 4) * U
    lam32 = float(np.float32(lam))
    oml = float(np.float32(1.0) - np.float32(lam))
    worst_sim = worst_pick = 0.0
    compared = 0
    for q in range(cand_id.shape[0]):
        S = sims_fp64(corpus, cnorm, cand_id[q]).numpy()
        r64 = rel[q].double().numpy()
        C = len(r64)
        avail = np.ones(C, bool)
        m = np.zeros(C)
        same_so_far = True
        for r in range(K):
            p = int(pos[q, r])
            assert 0 <= p < C and avail[p] and int(ids[q, r]) == int(cand_id[q, p]), (q, r, p)
            v = lam32 * r64 - oml * m
            e = oml * e_sim * (r > 0) + 3 * U * (lam32 * np.abs(r64) + oml * np.abs(m))
            d_sim = abs(float(ms[q, r]) - m[p])
            assert d_sim <= (e_sim if r else 0.0), (q, r, d_sim, e_sim)
            worst_sim = max(worst_sim, d_sim / e_sim)
            order = sorted(np.flatnonzero(avail), key=lambda i: (-v[i], i))
            b = order[0]
            tol = 2 * max(e[p], e[b])
            assert v[p] >= v[b] - tol, (q, r, p, b, v[p], v[b], tol)
            worst_pick = max(worst_pick, (v[b] - v[p]) / tol)
            # (the reference runs on its own: once it took another candidate in a near-tie, its later
            # rounds answer another question and are not compared)
            if ref_ids is not None and same_so_far:
                if len(order) == 1 or v[b] - v[order[1]] > 2 * max(e[b], e[order[1]]):
                    assert p == b and int(ref_ids[q, r]) == int(ids[q, r]), (q, r, p, b, int(ref_ids[q, r]))
                    compared += 1
                same_so_far = int(ref_ids[q, r]) == int(ids[q, r])
            avail[p] = False
            m = S[:, p].copy() if r == 0 else np.maximum(m, S[:, p])
    return worst_sim, worst_pick, compared
