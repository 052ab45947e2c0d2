"""csrc/knn.hip and the scores path of csrc/skinny_gemm.hip on the GPU, both routes of ``knn_topk``
(fused=False: weight-streaming GEMM scores + chunked top-k; fused=True: the single-pass MFMA kernel):
the exact probes of tests/knn_probes.py bit for bit and with no tolerance (every launch twice: the
same bits on every run), full coverage of every (query, row) pair through the rotating window,
``knn_merge`` alone against its model, the NaN and refusal conventions, position independence, and
a random tier within the derived bound B of knn_probes.random_case.

Measured on an MI355X (`pytest -s` prints it): the exact tier passes with zero tolerance on both
routes.  Random tier, worst |score - fp64| / B per shape (N, D), GEMM route / fused route: (777, 256)
0.008 / 0.005; (3000, 128) 0.010 / 0.010; (2000, 512) 0.003 / 0.003; (1000, 768) 0.002 / 0.002;
(5000, 1024) 0.001 / 0.001; (1300, 384) 0.003 / 0.003; every id equal to the fp64 order's.  The sharded
scan and the batch composition give the same bits on both routes (docs/kernels.md, kNN exactness).
"""
import pytest
import torch

import knn_probes as P
from llm_kubernetes_minikube_sharp4dev_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
FUSED_D = (128, 256, 384, 512, 768, 1024)
DEFAULT_D = (64, 192, 320) + FUSED_D
N0, NQ0 = 2 * P.ROWS + 37, 33  # the full-coverage shape
ROUTE = {False: "GEMM scores + chunked top-k", True: "fused", None: "route chosen by knn_topk"}


class OnDevice:
    """Uploads each probe tensor once (the rotation reuses the corpus and the queries)."""

    def __init__(self):
        self.kept = {}

    def __call__(self, t):
        if id(t) not in self.kept:
            self.kept[id(t)] = (t, t.to(DEV).contiguous())
        return self.kept[id(t)][1]


def launch(hip, a, fused):
    return hip.knn_topk(*a) if fused is None else hip.knn_topk(*a, fused)


def run(hip, L, fused, dev):
    """One probe launch: equal to the model bit for bit, and to itself when launched again."""
    a = (dev(L.c), dev(L.cn), dev(L.q), dev(L.qn), L.K)
    s, i = launch(hip, a, fused)
    s2, i2 = launch(hip, a, fused)
    P.check_exact(s, i, L, ROUTE[fused])
    assert P.same((s, i), (s2, i2)), f"{ROUTE[fused]} {L.what}: two launches differ"
    return s, i


def run_coverage(hip, kind, N, D, nq, fused, windows=None, K=P.WIN):
    """The rotation of one family; every pair that must be observed came back in some list."""
    launches, must = P.coverage(kind, N, D, nq, windows, K)
    dev, seen = OnDevice(), torch.zeros(nq, N, dtype=torch.bool)
    for L in launches:
        _, i = run(hip, L, fused, dev)
        seen |= P.observed(i, N)
    if K == P.WIN:
        unobserved = float((must & ~seen).double().mean())
        assert unobserved == 0.0, f"{kind} N={N} D={D} nq={nq}: {unobserved:.3%} of the pairs were never returned"


# ------------------------------------------------------------------ 1, 2. full coverage, every D
@pytest.mark.parametrize("D, fused", [(D, False) for D in DEFAULT_D] + [(D, True) for D in FUSED_D])
def test_full_coverage_every_width(hip, D, fused):
    for kind in ("S", "H"):
        run_coverage(hip, kind, N0, D, NQ0, fused)


@pytest.mark.parametrize("nq, fused", [(n, f) for n in (1, 31, 32, 33, 64) for f in (False, True)]
                         + [(n, False) for n in (65, 128, 129, 192, 193, 256)] + [(257, None)])
def test_full_coverage_query_counts(hip, nq, fused):
    """The query tiles of the fused kernel and the M-tile arms 4 / 8 / 12 / 16 of the scores GEMM;
    nq = 257 without ``fused`` takes the fused route by itself (test_refusals shows that it does)."""
    for kind in ("S", "H"):
        run_coverage(hip, kind, N0, 128, nq, fused)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("N", [1, 3, 127, 128, 129, 130, 255, 256, 257, 4095, 4096, 4097, 4096 + 131])
def test_corpus_edges(hip, N, fused):
    """The 128-row GEMM tile, the 256-row fused block, the 4096-row chunk, N % 4 != 0 (scalar store arm)
    against N % 4 == 0 (vector arm): the first, the last and every edge's window."""
    for kind in ("S", "H"):
        run_coverage(hip, kind, N, 128, 5, fused, P.edge_windows(N))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("N", [1, 3, 63, P.ROWS + 5, N0])
def test_small_and_large_k(hip, N, fused):
    """K 1, 10, 64; K > N; a tail block with fewer than K valid rows."""
    dev = OnDevice()
    c, q, dot = P.sign_case(N, 128, 5, seed=9)
    one = torch.ones(5)
    for K in (1, 10, 64):
        run(hip, P.Launch(f"S cn = 1, K={K}", c, torch.ones(N), q, one, K, dot), fused, dev)
        for L in P.rotation(f"S K={K}", c, q, dot, P.edge_windows(N), K):
            run(hip, L, fused, dev)


# ------------------------------------------------------------------ 3. epilogue
@pytest.mark.parametrize("fused", [False, True])
def test_epilogue(hip, fused):
    """eps once and inside the denominator, the correctly rounded division, cn = 0, zero rows and
    queries, qn * cn = +inf."""
    dev = OnDevice()
    for L in P.epilogue():
        if L.what.startswith("3b"):
            assert P.division_separates(L)
        run(hip, L, fused, dev)


# ------------------------------------------------------------------ 4. ties
@pytest.mark.parametrize("fused", [False, True])
def test_tie_plateaus(hip, fused):
    dev = OnDevice()
    launches, rows = P.ties()
    for L in launches:
        s, i = run(hip, L, fused, dev)
    s, i = run(hip, launches[0], fused, dev)
    for j, r in rows.items():  # (what the model says, spelled out)
        k = min(P.WIN, len(r))
        assert i[j, :k].tolist() == sorted(r)[:k] and len(set(P.bits(s[j, :k]).tolist())) == 1


# ------------------------------------------------------------------ 5. position independence
def _sharded(hip, r, cuts, fused):
    c, cn, q, qn = (r[k].to(DEV) for k in ("c", "cn", "q", "qn"))
    ps, pi = [], []
    for a, b in cuts:
        s, i = hip.knn_topk(c[a:b], cn[a:b], q, qn, r["K"], fused)
        ps.append(s)
        pi.append(torch.where(i >= 0, i + a, i))
    return ops.knn_merge(torch.cat(ps, dim=1), torch.cat(pi, dim=1), r["K"])


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("N, D, cuts", [
    (3000, 128, [[(0, 1000), (1000, 3000)], [(0, 0), (0, 7), (7, 3000)], [(0, 131), (131, 2179), (2179, 3000)]]),
    (5000, 1024, [[(0, 4097), (4097, 5000)], [(0, 300), (300, 300), (300, 5000)], [(0, 4991), (4991, 5000)]]),
])
def test_sharded_scan_equals_the_single_scan(hip, N, D, cuts, fused):
    """randn data, no tolerance: the claim is equality.  Shards at arbitrary cuts (an empty one, one
    shorter than K), ids offset, merged by knn_merge: bit for bit the single scan.  Holds on both
    routes on the MI355X."""
    r = P.random_case(N, D)
    whole = _sharded(hip, r, [(0, N)], fused)
    assert P.same(whole, hip.knn_topk(*(r[k].to(DEV) for k in ("c", "cn", "q", "qn")), r["K"], fused))
    for cut in cuts:
        assert P.same(_sharded(hip, r, cut, fused), whole), f"{ROUTE[fused]}: shards {cut} differ from the single scan"


@pytest.mark.parametrize("fused", [False, True])
def test_batch_composition(hip, fused):
    """A query alone, and inside batches of 40, 100, 160 and 200 (the M-tile arms 4, 8, 12, 16 of the
    scores GEMM; 2 to 7 query tiles of the fused kernel): the same bits.  Holds on both routes."""
    r = P.random_case(3000, 128)
    g = torch.Generator().manual_seed(5)
    q = torch.randn(200, 128, generator=g).to(P.BF)
    qn = q.double().norm(dim=1).float().to(DEV)
    q, c, cn = q.to(DEV), r["c"].to(DEV), r["cn"].to(DEV)
    full = hip.knn_topk(c, cn, q, qn, 10, fused)
    for n in (40, 100, 160):
        part = hip.knn_topk(c, cn, q[:n], qn[:n], 10, fused)
        assert P.same(part, (full[0][:n], full[1][:n])), f"{ROUTE[fused]}: batch of {n} against batch of 200"
    for j in (0, 5, 39, 40, 77, 150, 199):
        one = hip.knn_topk(c, cn, q[j:j + 1], qn[j:j + 1], 10, fused)
        assert P.same(one, (full[0][j:j + 1], full[1][j:j + 1])), f"{ROUTE[fused]}: query {j} alone against batch of 200"


# ------------------------------------------------------------------ 6. knn_merge alone
@pytest.mark.parametrize("ncand", [1, 63, 64, 255, 256, 257, 1000])
def test_merge_alone(hip, ncand):
    """Against knn_probes.merge_model: id < 0 skipped whatever its score, NaN absent, ties in other
    waves and strides, ids up to 2^31 - 2, pads when K exceeds the valid candidates.  A (-inf, id >= 0)
    candidate is an ordinary one: returned as (-inf, id) after every finite score, before the pads."""
    for nq in (1, 33):
        cs, ci = P.merge_case(nq, ncand)
        ds, di = cs.to(DEV), ci.to(DEV)
        for K in (1, 10, 64):
            want = P.merge_model(cs, ci, K)
            got = hip.knn_merge(ds, di, K)
            bad = (P.bits(got[0].cpu()) != P.bits(want[0])) | (got[1].cpu() != want[1])
            assert not bool(bad.any()), (f"knn_merge nq={nq} ncand={ncand} K={K}: first wrong slot "
                                         f"{tuple(bad.nonzero()[0].tolist())}: got ({got[0].cpu()[bad][0]}, "
                                         f"{got[1].cpu()[bad][0]}), want ({want[0][bad][0]}, {want[1][bad][0]})")
            assert P.same(hip.knn_merge(ds, di, K), got) and P.same(ops.knn_merge(ds, di, K), got)
            assert P.same(ops.knn_merge(cs, ci, K), want)  # the CPU path


# ------------------------------------------------------------------ 7. non-finite scores
@pytest.mark.parametrize("fused", [False, True])
def test_nan_scores_are_absent(hip, fused):
    """A NaN score is never better than anything: the row is left out, a NaN query gets pads; the
    reference (ops.reference.stable_topk) says the same."""
    dev = OnDevice()
    for L in P.nan_launches():
        s, i = run(hip, L, fused, dev)
        assert P.ROWS + 3 not in i[0].tolist() and i[1].tolist() == [-1] * L.K
        rs, ri = ops.reference.knn_topk(L.c, L.cn, L.q, L.qn, L.K)
        assert torch.equal(ri, i.cpu())


# ------------------------------------------------------------------ 8. refusals and empties
def test_refusals_raise_before_any_launch(hip):
    c, q, _ = P.sign_case(300, 128, 3)
    c, q = c.to(DEV), q.to(DEV)
    cn, qn = torch.ones(300, device=DEV), torch.ones(3, device=DEV)

    def bf(*shape):
        return torch.zeros(*shape, dtype=P.BF, device=DEV)

    unsupported = r"knn_partial: unsupported shape/config \(code -2\)"
    for fused in (False, True):
        with pytest.raises(RuntimeError, match="dimension mismatch"):
            hip.knn_topk(c, cn, bf(3, 256), qn, 5, fused)
        with pytest.raises(RuntimeError, match=unsupported):
            hip.knn_topk(bf(300, 96), cn, bf(3, 96), qn, 5, fused)
        for K in (0, 65):
            with pytest.raises(RuntimeError, match=r"K in \[1, 64\]"):
                hip.knn_topk(c, cn, q, qn, K, fused)
        with pytest.raises(RuntimeError, match="norm shapes"):
            hip.knn_topk(c, cn[:-1], q, qn, 5, fused)
        with pytest.raises(RuntimeError, match="norm shapes"):
            hip.knn_topk(c, cn, q, torch.ones(4, device=DEV), 5, fused)
        with pytest.raises(RuntimeError, match="corpus must be contiguous"):
            hip.knn_topk(bf(300, 256)[:, :128], cn, q, qn, 5, fused)
        with pytest.raises(RuntimeError, match="queries must be contiguous"):
            hip.knn_topk(c, cn, bf(3, 256)[:, :128], qn, 5, fused)
        with pytest.raises(RuntimeError, match="cnorm must be contiguous"):
            hip.knn_topk(c, torch.ones(600, device=DEV)[::2], q, qn, 5, fused)
        with pytest.raises(RuntimeError, match="corpus must be bfloat16"):
            hip.knn_topk(c.float(), cn, q, qn, 5, fused)
    with pytest.raises(RuntimeError, match=unsupported):
        hip.knn_topk(bf(300, 320), cn, bf(3, 320), qn, 5, True)
    # the width that only the default route takes shows the route: 256 queries pass, 257 go to the
    # fused kernel by themselves and are refused there
    s, i = hip.knn_topk(bf(300, 320), cn, bf(256, 320), torch.ones(256, device=DEV), 5)
    assert i[255].tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(RuntimeError, match=unsupported):
        hip.knn_topk(bf(300, 320), cn, bf(257, 320), torch.ones(257, device=DEV), 5)


@pytest.mark.parametrize("fused", [False, True])
def test_empty_corpus_and_no_queries_return_pads(hip, fused):
    for N, nq in ((0, 3), (300, 0), (0, 0)):
        s, i = hip.knn_topk(torch.zeros(N, 128, dtype=P.BF, device=DEV), torch.ones(N, device=DEV),
                            torch.zeros(nq, 128, dtype=P.BF, device=DEV), torch.ones(nq, device=DEV), 7, fused)
        assert s.shape == (nq, 7) and i.shape == (nq, 7) and s.dtype == torch.float32 and i.dtype == torch.int32
        assert bool((s == P.NEG_INF).all()) and bool((i == -1).all())


# ------------------------------------------------------------------ random tier
@pytest.mark.parametrize("N, D", P.RANDOM_SHAPES)
def test_random_tier_within_the_derived_bound(hip, N, D):
    r = P.random_case(N, D)
    assert r["unpinned"] <= P.UNPINNED_CAP
    a = tuple(r[k].to(DEV) for k in ("c", "cn", "q", "qn"))
    for fused in (False, True):
        s, i = hip.knn_topk(*a, r["K"], fused)
        ratio = P.check_random(s, i, r, f"{ROUTE[fused]} N={N} D={D}")
        differ = int((i.cpu().long() != r["order"][:, : r["K"]]).sum())
        print(f"knn_topk N={N} D={D} nq={P.RANDOM_NQ} K={r['K']} {ROUTE[fused]}: worst |score - fp64| / B = {ratio:.3f}, "
              f"unpinned share {r['unpinned']:.2%}, {differ} ids differ from the fp64 order")
        assert P.same(hip.knn_topk(*a, r["K"], fused), (s, i))
