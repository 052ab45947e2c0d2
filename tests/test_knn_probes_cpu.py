"""tests/knn_probes.py on the CPU: the probes are sensitive (every mutant of the model changes a
returned bit pattern or id of some probe), full coverage leaves no (query, row) pair unobserved, the
builders' operands are exact, and the random tier's cap holds for the float64 reference alone."""
import pytest
import torch

import knn_probes as P
from llm_kubernetes_minikube_sharp4dev_amd import ops

N0, NQ0 = 2 * P.ROWS + 37, 33  # the full-coverage shape


@pytest.fixture(scope="module")
def probes():
    """The launches the mutants are tried on: full coverage of both families at D = 128 (S also with a
    partial last 128-tile whose window ends at the last row), the epilogue probes, the ties."""
    out = []
    for kind in ("S", "H"):
        out += P.coverage(kind, N0, 128, NQ0)[0]
    out += P.epilogue() + P.ties()[0]
    return out


def test_operands_survive_bf16_and_dots_stay_below_2_24(probes):
    for L in probes + P.nan_launches() + P.coverage("H", N0, 1024, NQ0)[0][:2] + P.coverage("S", 131, 64, 5)[0][:2]:
        for t in (L.c, L.q):
            fin = torch.nan_to_num(t.float(), nan=0.0)
            assert t.dtype == P.BF and torch.equal(fin.to(P.BF).float(), fin)
            assert float(fin.abs().max()) <= 125
        d = L.dot[torch.isfinite(L.dot)]
        assert float(d.abs().max()) < 2 ** 24 and torch.equal(d, d.round())
        assert torch.equal(torch.nan_to_num(L.dot), torch.nan_to_num(L.q.double() @ L.c.double().t()))
        P.denominators(L.cn, L.qn)  # asserts that qn * cn is exact in f32 (or overflows)


@pytest.mark.parametrize("kind, D", [("S", 128), ("H", 128), ("S", 64), ("S", 1024), ("H", 320), ("H", 1024)])
def test_full_coverage_leaves_no_pair_unobserved(kind, D):
    launches, must = P.coverage(kind, N0, D, NQ0)
    assert len(launches) == 2 * 9 * len(P.hot_offsets(N0, D) if kind == "H" else [0])
    seen = torch.zeros(NQ0, N0, dtype=torch.bool)
    for L in launches:
        s, i = P.model(L)
        assert bool((i >= 0).all()), "every slot of a full-coverage launch holds a row"
        seen |= P.observed(i, N0)
    unobserved = float((must & ~seen).double().mean())
    assert unobserved == 0.0, f"{unobserved:.3%} of the pairs never appear in a returned list"
    if kind == "S":
        assert bool(must.all())
    else:  # H: only the pattern's zeros (one k in 251) have nothing to show
        assert float((~must).double().mean()) < 0.01


def test_edge_windows_straddle_every_edge():
    for N in (1, 3, 127, 128, 129, 130, 255, 256, 257, 4095, 4096, 4097, 4096 + 131):
        w = P.edge_windows(N)
        assert w[0][0] == 0 and max(b for _, b in w) == N and all(0 < b - a <= P.WIN for a, b in w)
        for t in (P.BN, P.ROWS, P.SCH):
            for e in range(t, N, t):
                if e in (t, (N - 1) // t * t):
                    assert any(a < e < b for a, b in w), (N, e)
        _, must = P.coverage("S", N, 128, 5, w)
        assert int(must[0].sum()) == len({n for a, b in w for n in range(a, b)})


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_every_mutant_changes_a_returned_bit(probes, mutant):
    caught = [L.what for L in probes if not P.same(P.model(L), P.model(L, mutant))]
    assert caught, f"no probe notices the mutant {mutant}"
    if mutant in ("no_eps", "eps_outside"):
        assert any(w.startswith("3a") for w in caught)
    if mutant == "trunc_div":
        assert any(w.startswith("3b") for w in caught)
    if mutant in ("ties_desc",):
        assert any(w.startswith("ties") for w in caught)
    if mutant in ("drop_row", "skip_chunk", "swap_lr4", "swap_qcol", "unclamped"):
        assert any(w.startswith("S ") for w in caught) and (mutant == "unclamped" or any(w.startswith("H ") for w in caught))


def test_unclamped_row_shows_at_every_partial_tile():
    for N in (1, 3, 127, 129, 130, 255, 257, 4095, 4097, 4096 + 131):
        launches, _ = P.coverage("S", N, 128, 5, P.edge_windows(N))
        assert any(int(P.model(L, "unclamped")[1].max()) == N for L in launches), N


def test_division_probe_tells_rounding_from_truncation():
    e = {L.what: L for L in P.epilogue()}
    for what in ("3b denominators 3, 5, 7, 11", "3b denominators 3, 5, 7, 11 at K = 10"):
        assert P.division_separates(e[what])
    # the power-of-two probes do not depend on the division's rounding
    L = P.coverage("S", N0, 128, NQ0)[0][0]
    assert not P.division_separates(L)


def test_epilogue_probe_values():
    e = {L.what: L for L in P.epilogue()}
    s, i = P.model(e["3c cn = 0 with a non-zero dot"])
    assert bool((i[:, 0] % 5 == 0).all()) and torch.equal(s[:, 0], (e["3c cn = 0 with a non-zero dot"].dot.gather(
        1, i[:, :1].long())[:, 0].float() / P.EPS32))
    L = e["3d zero row and zero query"]
    s, i = P.model(L)
    assert i[2].tolist() == list(range(L.K)) and P.bits(s[2]).tolist() == [0] * L.K  # +0.0
    for j in (0, 1, 3, 4):
        at = [i[j].tolist().index(n) for n in (70, P.ROWS + 9) if n in i[j].tolist()]
        assert all(P.bits(s[j])[p] == 0 for p in at)
    full = P.topk_model(P.model_scores(L.dot, L.cn, L.qn), L.c.shape[0])
    p70 = full[1][0].tolist().index(70)
    assert full[1][0, p70 + 1] == P.ROWS + 9 and float(full[0][0, p70 - 1]) > 0 > float(full[0][0, p70 + 2])
    L = e["3e qn * cn = +inf"]
    s, i = P.model(L)
    for j in (0, 3):
        assert i[j].tolist() == list(range(L.K)) and bool((s[j] == 0).all())
        assert set(P.bits(s[j]).tolist()) == {0, -2 ** 31}  # both zeros occur, and tie


def test_tie_plateaus_return_the_lowest_ids_in_order():
    launches, rows = P.ties()
    L = launches[0]
    s, i = P.model(L)
    for j, r in rows.items():
        k = min(L.K, len(r))
        assert i[j, :k].tolist() == sorted(r)[:k] and len(set(P.bits(s[j, :k]).tolist())) == 1
    assert len(rows[0]) > P.WIN and min(rows[0]) < P.BN < max(rows[0])
    assert {n // P.SCH for n in rows[1]} == {0, 1} and len({n // P.ROWS for n in rows[1]}) >= 4
    # ties of their own below the plateau: equal scores at neighbouring positions, ids ascending
    eq = s[4, :-1] == s[4, 1:]
    assert bool(eq.any()) and bool((i[4, :-1][eq] < i[4, 1:][eq]).all())
    s, i = P.model(launches[-1])
    M = launches[-1].c.shape[0]
    assert M % P.ROWS < P.WIN and i[2, :30].tolist() == list(range(M - 30, M))


def test_nan_is_absent_in_the_model_and_in_the_reference():
    for L in P.nan_launches():
        s, i = P.model(L)
        assert torch.equal(i[1], torch.full((L.K,), -1, dtype=torch.int32)) and bool((s[1] == P.NEG_INF).all())
        assert P.ROWS + 3 not in i.tolist()[0] and bool((i[0] >= 0).all())
        assert L.K < P.WIN or int(i[0].max()) > P.ROWS + 3  # the list reaches past the NaN row
        # ops.reference: the same ids (its scores are float64 quotients rounded once more)
        rs, ri = ops.reference.knn_topk(L.c, L.cn, L.q, L.qn, L.K)
        assert torch.equal(ri, i) and torch.equal(rs, s)
    sc = torch.tensor([[1.0, float("nan"), 3.0, float("nan")], [float("nan")] * 4])
    rs, ri = ops.reference.stable_topk(sc, 3)
    assert ri.tolist() == [[2, 0, -1], [-1, -1, -1]] and rs[0].tolist() == [3.0, 1.0, P.NEG_INF]


@pytest.mark.parametrize("ncand", [1, 63, 64, 255, 256, 257, 1000])
def test_merge_model_and_cpu_path(ncand):
    for nq in (1, 33):
        cs, ci = P.merge_case(nq, ncand)
        for K in (1, 10, 64):
            ws, wi = P.merge_model(cs, ci, K)
            gs, gi = ops.knn_merge(cs, ci, K)
            assert P.same((gs, gi), (ws, wi))
            valid = ((ci >= 0) & ~torch.isnan(cs)).sum(1)
            assert torch.equal((wi >= 0).sum(1), valid.clamp(max=K))
            assert bool((wi[:, 1:][wi[:, 1:] >= 0] != wi[:, :-1][wi[:, 1:] >= 0]).all())
            if ncand >= 63:
                assert not P.same(P.merge_model(cs, ci, K, keep_negative=True), (ws, wi)), "merge keeping id < 0"
        if ncand >= 63:  # the (-inf, id >= 0) candidate is the last hit before the pads
            ws, wi = P.merge_model(cs, ci, 64)
            last = (wi >= 0).sum(1) - 1
            if int(last[0]) < 63:
                assert float(ws[0, last[0]]) == P.NEG_INF and int(wi[0, last[0]]) == int(ci[0, 10])
    assert int(ci.max()) == P.ID_MAX or ncand == 1


@pytest.mark.parametrize("N, D", P.RANDOM_SHAPES)
def test_random_tier_cap_holds_for_the_reference_alone(N, D):
    r = P.random_case(N, D)
    print(f"random tier N={N} D={D}: unpinned share {r['unpinned']:.2%}, bound {float(r['B'].min()):.2e} .. "
          f"{float(r['B'].max()):.2e}")
    assert r["unpinned"] <= P.UNPINNED_CAP
    assert 1e-6 < float(r["B"].gather(1, r["order"]).max()) < 1e-4
    # the float64 reference, rounded to f32, passes its own check; a single swap of a pinned pair,
    # a repeated id or a score one bound off does not
    i = r["order"][:, : r["K"]].int()
    s = r["s64"].gather(1, i.long()).float()
    assert P.check_random(s, i, r) <= 1.0
    j, p = (int(v) for v in (r["pinned"][:, :-1] & r["pinned"][:, 1:]).nonzero()[0])
    bad = i.clone()
    bad[j, p], bad[j, p + 1] = i[j, p + 1], i[j, p]
    with pytest.raises(AssertionError):
        P.check_random(s, bad, r)
    bad = i.clone()
    bad[0, 1] = bad[0, 0]
    with pytest.raises(AssertionError):
        P.check_random(s, bad, r)
    off = s.clone()
    off[3, 2] += 2.5 * float(r["B"][3, i[3, 2]])
    with pytest.raises(AssertionError):
        P.check_random(off, i, r)
