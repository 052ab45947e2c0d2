"""CPU checks of tests/sampler_probes.py, the model the exact sampler tests compare the kernels of
csrc/sampling.hip with: the stream against an independent integer implementation, the model against
ops.reference where both are exact, the committed u == 1 tuples, the tolerances against what their
emulations measure, and -- the reason these inputs were chosen -- that each of seven plausible kernel
mistakes changes the expected token of a probe row, while the random rows stay pinned often enough."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_probes as P  # noqa: E402

from llm_kubernetes_minikube_sharp4dev_amd.ops import reference as ref  # noqa: E402

M64 = (1 << 64) - 1


def _hash3_int(a, b, c):
    x = ((a << 32) ^ (b * 0x9E3779B97F4A7C15) ^ c) & M64
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    x ^= x >> 31
    return x >> 32


def test_hash3_and_fold_against_python_integers():
    rng = np.random.default_rng(0)
    a, b, c = (rng.integers(0, 1 << 32, 500) for _ in range(3))
    a[:3], b[:3], c[:3] = [0, 0xFFFFFFFF, 1], [0, 0xFFFFFFFF, 0], [0, 0xFFFFFFFF, 0x80000000]
    assert P.hash3(a, b, c).tolist() == [_hash3_int(int(x), int(y), int(z)) for x, y, z in zip(a, b, c)]
    assert int(P.hash3(5, -1, 7)[0]) == _hash3_int(5, 0xFFFFFFFF, 7)  # a negative request seed is its 32 bits
    assert int(P.hash3(0xFFFFFFFF + 3, 1, 2)[0]) == _hash3_int(2, 1, 2)  # seed + row wraps at 2^32
    assert P.fold(123) == 123 and P.fold(0x1234567890) == 0x34567890 ^ 0x12
    assert P.fold((1 << 63) | 5) == 5  # ops.select_tokens / ops.sample pass 63 bits down


def test_uniform_cap_changes_one_value_of_2_24():
    h = np.arange(1 << 24, dtype=np.uint32) << np.uint32(8)
    raw, cap = P.uniform(h, cap=False), P.uniform(h)
    assert raw.dtype == np.float32 and raw[0] == np.float32(2.0 ** -25) and raw.min() > 0
    assert np.flatnonzero(raw != cap).tolist() == [0xFFFFFF] and raw[-1] == 1.0 and cap[-1] == P.U_CAP < 1
    assert np.array_equal(P.uniform(h | np.uint32(0xFF)), cap)  # the low 8 bits play no part
    assert (np.diff(cap.astype(np.float64)) >= 0).all()
    # the kernels form u with one FMA, h * 2^-24 + 2^-25 (exact in float64), rounded once: the same bits
    fma = ((h >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 + 2.0 ** -25).astype(np.float32)
    assert np.array_equal(fma, raw)


def test_committed_tuples_hash_to_the_top_value():
    for seed, row, step, tok in P.U1_GUMBEL:
        assert int(P.gumbel_hash(seed, row, step, tok)[0]) >> 8 == 0xFFFFFF
        l = np.zeros(2048, np.float32)
        l[tok] = -50.0
        assert P.gumbel(l, 1.0, seed, row, step, cap=False) == {tok}  # the parent's kernel: +inf noise wins
        assert tok not in P.gumbel(l, 1.0, seed, row, step)
    for seed, rseed, hl in P.U1_SAMPLE:
        assert int(P.sample_hash(seed, rseed, hl)[0]) >> 8 == 0xFFFFFF
    for seed, rseed, hl in P.INT_U_1024:
        u = P.uniform(P.sample_hash(seed, rseed, hl))[0] * np.float32(1024)
        assert u == math.floor(u)
    assert P.search_int_u(123, 0, 2000) == [1976] and P.search_u1_gumbel(0x1234567890, 3, 2048, 300) == (263, 1898)
    assert sum(s == 123 for s, _, _ in P.INT_U_1024) == 2 and P.U1_SAMPLE[0][0] == 123  # rows 0..2 of a plateau case


# ---------------------------------------------------------------- the model against ops.reference
def test_order_matches_the_reference_sort():
    rng = np.random.default_rng(1)
    l = np.round(rng.standard_normal(300) * 2).astype(np.float32)  # many ties
    l[[3, 200]], l[[9, 100]] = -0.0, 0.0
    for K in (1, 7, 299, 300):
        assert P.order(l, K).tolist() == ref._topk_stable(torch.from_numpy(l), K)
    z = np.full(8, -5.0, np.float32)
    z[0], z[5] = -0.0, 0.0
    assert P.order(z, 2).tolist() == [0, 5] == ref._topk_stable(torch.from_numpy(z), 2)
    assert P.order(z, 2, mut=("zero_order",)).tolist() == [5, 0]
    l[10:290] = -np.inf
    assert P.order(l, 40).tolist() == ref._topk_stable(torch.from_numpy(l), 20)  # 20 finite entries: k_eff
    assert P.chain(np.full(9, -np.inf, np.float32), P.prm_rows(1)[0], 1, 0) == {0}
    assert [P.k_of(t, k, V) for t, k, V in ((0, 40, 99), (1, 0, 5000), (1, 0, 7), (1, 5000, 4097), (1, 40, 99), (1, 40, 8))] \
        == [1, 1024, 7, 1024, 40, 8]


def test_kept_count_on_the_plateaus():
    """floor(top_p * K) + 1 clamped to K in the model; the reference's draws stay inside that prefix."""
    for K in P.PLATEAU_K:
        case = P.plateau_case(K, 8)
        od = P.order(case.logits[0], K)
        rows = range(3, 43)
        for r in rows:
            info = {}
            (tok,) = P.chain(case.logits[r], case.prm[r], case.seed, int(case.hl[r]), exact=True, info=info)
            nk = min(int(math.floor(float(P.parse(case.prm[r])["top_p"]) * K)) + 1, K)
            assert info["nkeeps"] == [nk] and tok == od[min(int(np.float32(info["u01"] * nk)), nk - 1)]
        sl = slice(3, 43)
        hist, hl = torch.from_numpy(case.hist.copy()), torch.from_numpy(case.hl.copy())
        prm = torch.from_numpy(case.prm[sl].copy())
        got = ref.sample(torch.from_numpy(case.logits[sl].copy()), prm, hist, hl, seed=case.seed)
        for r, t in zip(rows, got.tolist()):
            nk = min(int(math.floor(float(P.parse(case.prm[r])["top_p"]) * K)) + 1, K)
            assert t in od[:nk]
    picks = {int(t) // 2 // 64 for (t,) in P.plateau_case(1024, 8).expected()}
    assert picks == set(range(16))  # the picks land in every wave of the scan


def test_greedy_ring_and_reset_match_the_reference():
    rng = np.random.default_rng(2)
    B, V, W = 24, 500, 16
    logits = np.round(rng.standard_normal((B, V)) * 3).astype(np.float32) / 2
    hist = rng.integers(0, 40, (B, W)).astype(np.int32)
    hl = rng.integers(0, 3 * W, B).astype(np.int32)
    prm = P.prm_rows(B, 8, 0.0, 40, 0.9, pen=1.5, last_n=np.take((5, -1, 0, 64), np.arange(B) % 4), reset=np.arange(B) % 5 == 0)
    case = P.Case("greedy", logits, prm, hl, W=W, hist=hist)
    h, n = torch.from_numpy(hist.copy()), torch.from_numpy(hl.copy())
    lg = torch.from_numpy(logits.copy())
    got = ref.sample(lg, torch.from_numpy(prm), h, n).tolist()
    assert [{t} for t in got] == case.expected()
    assert np.array_equal(lg.numpy(), np.stack([case.edited(r) for r in range(B)]))
    for r in range(B):
        assert int(n[r]) == case.position(r) + 1 and int(h[r, case.position(r) % W]) == got[r]
        assert case.position(r) == (0 if r % 5 == 0 else hl[r])


# ---------------------------------------------------------------- tolerances
def test_eps_constants_are_the_measured_ones():
    eps = max(P.measure_eps(l[r], prm[r]) for _, l, prm, _ in P.random_cases() for r in range(P.RANDOM_B))
    for row, k, _ in P.radix_rows().values():
        eps = max(eps, P.measure_eps(row, P.prm_rows(1, 8, 1.0, k, 1.0)[0]))
    temps = P.gumbel_temps()
    eps_g = max(P.measure_eps_g(P.gumbel_logits(V)[r], temps[r], seed, r, step) for V in P.GUMBEL_V for seed in P.GUMBEL_SEEDS
                for step in P.GUMBEL_STEPS for r in range(P.GUMBEL_B) if temps[r] > 0)
    print(f"measured eps {eps:.4e} eps_g {eps_g:.4e}")
    assert eps <= P.MEASURED["eps"] <= 1.02 * eps and eps_g <= P.MEASURED["eps_g"] <= 1.02 * eps_g
    assert P.EPS == 2 * P.MEASURED["eps"] and P.EPS_G == 2 * P.MEASURED["eps_g"]
    # the scan's emulation keeps integers exact and is an inclusive prefix
    assert np.array_equal(P.scan32(np.ones(1024, np.float32)), np.arange(1, 1025, dtype=np.float32))


# ---------------------------------------------------------------- mutants
WHERE = {"topp_lt": lambda: [P.plateau_case(8, 8)], "pick_ge": lambda: [P.plateau_case(1024, 8)],
         "pos_mod_w": lambda: [P.position_case()], "row_hash": lambda: [P.placement_cases()[1]],
         "zero_order": lambda: [P.zeros_case()], "drop_wave1": lambda: [P.plateau_case(1024, 12), P.sizes_case(1023)],
         "k_unclamped": lambda: [P.sizes_case(1025), P.sizes_case(4097)]}


@pytest.mark.parametrize("mut", P.MUTANTS)
def test_each_mistake_changes_an_expected_token(mut):
    for case in WHERE[mut]():
        want, wrong = case.expected(), case.expected(mut=(mut,))
        assert all(len(s) == 1 for s in want)
        changed = [r for r, (a, b) in enumerate(zip(want, wrong)) if a.isdisjoint(b)]
        assert changed, (mut, case.name)
    if mut == "pick_ge":  # only the rows whose u * 1024 is an integer tell ">" from ">="
        assert changed == [0, 1]
    if mut == "row_hash":  # row 37 of 64 changes, row 0 of 1 cannot
        one = P.placement_cases()[0]
        assert 37 in changed and one.expected() == one.expected(mut=(mut,))


def test_exact_cases_are_pinned_and_well_formed():
    for case in P.exact_cases():
        assert all(len(s) == 1 for s in case.expected()), case.name
        assert len(set(case.prm[:, 5].tolist())) == len(case.prm)  # one slot per row
    pos = P.position_case()
    toks = [t for (t,) in pos.expected()]
    assert len(set(toks[:-1])) == len(P.POS_HL) and toks[-1] == toks[0]
    one, many = P.placement_cases()
    assert one.expected()[0] == many.expected()[37]
    for name, (row, k, _) in P.radix_rows().items():
        assert len(row) == 8192 and P.needs_radix(row, k), name
    assert not P.needs_radix(P.plateau_case(1024, 8).logits[0], 1024)
    under = P.underflow_case(8)
    assert all(under.logits[0][t] == 3.0 for (t,) in under.expected())
    assert np.exp(np.float32(-200.0)) == 0  # e of the lower level in float32


# ---------------------------------------------------------------- caps on the unpinned share
def test_unpinned_share_of_the_random_rows():
    for i in range(len(P.random_cases())):
        case = P.random_case(i)
        share = sum(len(s) > 1 for s in case.expected()) / P.RANDOM_B
        assert share <= P.unpinned_cap(case.prm[0], case.logits.shape[1]), (case.name, share)
    pen = P.penalty_case()
    assert sum(len(s) > 1 for s in pen.expected()) <= 0.02 * P.RANDOM_B
    assert any(P.order(pen.edited(r), 8).tolist() != P.order(pen.logits[r], 8).tolist() for r in range(8))
    for name, (_, _, exact) in P.radix_rows().items():
        if not exact:
            assert sum(len(s) > 1 for s in P.radix_case(name).expected()) <= 0.10 * 32, name


def test_unpinned_share_of_the_gumbel_rows():
    temps, rows, unpinned = P.gumbel_temps(), 0, 0
    assert set(temps.tolist()) == set(P.GUMBEL_TEMPS)
    for V in P.GUMBEL_V:
        _, allowed = P.allowed_plan(P.GUMBEL_B, V)
        for seed in P.GUMBEL_SEEDS:
            for step in P.GUMBEL_STEPS:
                for r in range(P.GUMBEL_B):
                    for ids in (None, allowed[r]):
                        rows += 1
                        unpinned += len(P.gumbel(P.gumbel_logits(V)[r], temps[r], seed, r, step, ids)) > 1
    assert unpinned <= 0.01 * rows, (unpinned, rows)
    # a greedy row takes the lowest id of the maximum, zeros of either sign equal
    z = np.asarray([-1.0, -0.0, 0.0, -3.0], np.float32)
    assert P.gumbel(z, 0.0, 1, 0, 0) == {1} and P.gumbel(z, 0.0, 1, 0, 0, allowed=[3, 2, 0]) == {2}
