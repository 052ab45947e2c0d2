"""tests/gemm_probes.py without a GPU: the builders' invariants, the float64 expectations against
int64 arithmetic, the tolerance constants against their measurement, and -- the point of the probes
-- that a blocked GEMM emulation with ONE injected fault fails the probe named for it."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_probes as P  # noqa: E402


# ---------------------------------------------------------------- builders
@pytest.mark.parametrize("K,cap", [(576, 0.0), (4096, 1e-3), (14336, 0.05)])
def test_dense_sign_is_exact_and_sensitive(K, cap):
    x, w = P.dense_sign(48, 256, K, 1.0, seed=K)
    assert x.dtype == P.BF and w.dtype == P.BF
    assert bool((x.float().abs() == 1).all()) and bool((w.float().abs() == 1).all())
    e = P.expect(x, w)
    share = P.assert_sensitive(e)
    assert share <= cap
    if K == 576:
        assert float(e.abs().max()) <= 128
    x2, w2 = P.dense_sign(48, 256, K, 1.0, seed=K)
    assert torch.equal(x, x2) and torch.equal(w, w2), "the generator is seeded"


@pytest.mark.parametrize("K", [64, 256, 576, 2048, 4096, 6144, 14336])
def test_epilogue_density_keeps_the_accumulator_small(K):
    d = P.epi_density(K)
    assert K * d <= 256
    x, w = P.dense_sign(64, 512, K, d, seed=1)
    assert set(w.float().unique().tolist()) <= {-1.0, 0.0, 1.0}
    e = P.expect(x, w)
    P.assert_acc_cap(e)
    assert float(e.abs().max()) >= 16, "the accumulators are not trivial"
    with pytest.raises(AssertionError):
        P.assert_acc_cap(e * 20)


@pytest.mark.parametrize("M,N,K", [(1, 256, 256), (2, 64, 256), (300, 64, 256), (40, 768, 576), (1300, 768, 576)])
def test_one_hot_covers_every_k_and_names_it(M, N, K):
    seen = torch.zeros(K, dtype=torch.bool)
    rows = max(M, N)
    for shift in P.hot_shifts(rows, K):
        x, w, k0, side = P.one_hot(M, N, K, shift)
        assert side == ("w" if N >= M else "x")
        hot = w if side == "w" else x
        other = x if side == "w" else w
        assert bool(((hot != 0).sum(1) == 1).all())
        assert set(hot.float().abs().unique().tolist()) <= {0.0, 1.0, 2.0}
        assert float(other.float().abs().max()) <= 127
        seen[k0] = True
        assert torch.equal(P.expect(x, w), P.one_hot_expect(x, w, k0, side))
    assert bool(seen.all()), "a k is never selected"
    for k in range(64, K, 64):  # both sides of every 64-element K-step
        assert seen[k - 1] and seen[k]


@pytest.mark.parametrize("K,S", [(64, 1), (128, 1), (128, 2), (256, 4), (512, 8), (1536, 2), (6144, 8)])
def test_rounding_separates_the_rounding_modes(K, S):
    pairs = P.split_pairs(K, S)
    ks = K // S
    for p in pairs:
        assert p[0] // ks != p[1] // ks or S == 1, "k1 and k2 in different splits"
        assert p[0] // 64 != p[1] // 64 or K == 64, "k1 and k2 in different K-steps"
        if len(p) == 3:
            assert p[2] // ks == p[0] // ks, "k3 in k1's split"
    two = [p for p in pairs if len(p) == 2]
    x, w = P.rounding(len(two), 192, K, two)
    assert bool((x.float().sum(1) == 2).all())
    big = w.float().abs().max(1).values
    assert bool(((big >= 256) & (big <= 510) & (big % 2 == 0)).all())
    e = P.expect(x, w)
    P.assert_rounding_separates(e)
    assert bool((e != e.round()).any()) and bool(((e % 2).abs() == 1).any()), "halves and exact ties"
    want = P.rbf(e)
    assert torch.equal(want.double(), P.round_bf16(e, "rne")), "torch's f32 -> bf16 is round-to-nearest-even"
    assert float(P.round_bf16(torch.tensor([257.0]))) == 256.0 and float(P.round_bf16(torch.tensor([259.0]))) == 260.0
    three = [p for p in pairs if len(p) == 3]
    x3, w3 = P.rounding(len(three), 192, K, three)
    assert bool((x3.float().sum(1) == 3).all())


def test_float64_expectation_equals_int64():
    for x, w in (P.dense_sign(33, 80, 320, 0.5, seed=3), P.one_hot(33, 320, 320)[:2], P.one_hot(400, 48, 320)[:2]):
        assert torch.equal(P.expect(x, w), (x.long() @ w.long().t()).double())
    x, w = P.rounding(6, 64, 256, P.split_pairs(256, 2))
    assert torch.equal(P.expect(x, w), ((2 * x.float()).long() @ (2 * w.float()).long().t()).double() / 4)


def test_exact_epilogues():
    K = 576
    x, w = P.dense_sign(20, 256, K, P.epi_density(K), seed=2)
    acc = P.expect(x, w)
    b = P.int_vector(256, -64, 64, 5)
    r = P.int_matrix(20, 256, -32, 32, 6)
    assert torch.equal(P.exp_bias(acc, b).double(), acc + b.double())  # |acc + b| <= 256: exact
    relu = P.exp_bias_relu(acc, b)
    assert bool((relu[(acc + b.double()) < 0] == 0).all()) and bool((relu >= 0).all())
    new, ss = P.exp_resid(acc, r)
    assert torch.equal(new.double(), acc + r.double())
    assert ss.shape == (1, 20) and torch.equal(ss[0], (acc + r.double()).pow(2).sum(1))
    assert float(ss.max()) < 2 ** 24
    # an accumulator bf16 does not hold: rounded before the residual is added
    big = torch.tensor([[257.0, 259.0]])
    new, _ = P.exp_resid(big, torch.tensor([[1.0, 1.0]]).to(P.BF))
    assert new.tolist() == [[256.0, 260.0]]  # 257 -> 256, + 1 -> 257 -> 256; 259 -> 260, + 1 -> 261 -> 260


# ---------------------------------------------------------------- tolerances
def test_tolerance_constants_match_their_measurement():
    got = P.measure_ulps()
    for kind, m in got.items():
        assert P.MEASURED[kind] == math.ceil(m * 1000 - 1e-9) / 1000, f"{kind}: measured {m}"
        assert P.ULPS[kind] == 2 * P.MEASURED[kind]


def test_emulations_give_exact_zeros():
    r = torch.arange(-192, 193, dtype=torch.float64)
    assert bool((P.emu_swiglu(r, torch.zeros_like(r)) == 0).all()), "SwiGLU with u == 0"
    assert bool((P.swiglu64(r, torch.zeros_like(r)) == 0).all())
    assert float(P.emu_gelu(torch.zeros(1))) == 0.0 and float(P.gelu64(torch.zeros(1, dtype=torch.float64))) == 0.0
    # elementwise: a wrong GELU of a negative input fails although the matrix holds large values
    e = torch.tensor([[200.0, -3.0]], dtype=torch.float64)
    good = P.emu_gelu(e).to(P.BF)
    P.check("gelu", good, P.gelu64(e), "gelu", floor=P.gelu_floor(e))
    bad = good.clone()
    bad[0, 1] = 0.0
    with pytest.raises(AssertionError):
        P.check("gelu", bad, P.gelu64(e), "gelu", floor=P.gelu_floor(e))
    with pytest.raises(AssertionError):  # an expected zero must be an exact zero
        P.check("swiglu", torch.tensor([[1e-30]]).to(P.BF), torch.zeros(1, 1, dtype=torch.float64), "swiglu")
    # position 0 rotates by (1, 0): exact
    cs = P.rope_table(38, 64)
    q = P.int_matrix(2, 4 * 64, -192, 192, 9).double()
    want, floor = P.rope_expect(q, torch.tensor([0, 0]), cs, 2, 1, 64, True, True)
    assert torch.equal(want, q) and float(floor[:, 3 * 64:].max()) == 0.0


# ---------------------------------------------------------------- sensitivity
def blocked_gemm(x, w, splits=1, store="rne", mutant=None, bias=None, relu=False):
    """A K-blocked (64 per step), split-K GEMM in f32 with a bf16 store into a sentinel-filled
    buffer; ``mutant`` injects one fault."""
    M, K = x.shape
    N = w.shape[0]
    nst = K // 64
    xs, ws = x.float(), w.float()
    parts = []
    for z in range(splits):
        acc = torch.zeros(M, N)
        for st in range(z * nst // splits, (z + 1) * nst // splits):
            sx = st
            if mutant == "swap_x" and st in (0, 2):
                sx = 2 - st
            xk, wk = xs[:, sx * 64:(sx + 1) * 64].clone(), ws[:, st * 64:(st + 1) * 64]
            if mutant == "chunk" and st == 2:
                xk[16:32, 24:32] = 0  # one 8-element chunk, one 16-row tile
            acc += xk @ wk.t()
            if mutant == "twice" and st == 1:
                acc[:, 64:128] += xk @ wk[64:128].t()  # one K-step twice for one column tile
            if mutant == "drop" and st == 133 // 64:
                acc[17, 133] -= xs[17, 133] * ws[133, 133]
        if mutant == "partial_bf16":
            acc = acc.to(P.BF).float()
        parts.append(acc)
    e = sum(parts).double()
    if bias is not None:
        if mutant == "bias_after":
            e = torch.relu(e) + bias.double()[None, :]
        else:
            e = P.round_bf16(e + bias.double()[None, :], "rne")
            e = torch.relu(e) if relu else e
    mode = {"trunc": "trunc", "half_away": "half_away"}.get(mutant, store)
    y = P.round_bf16(e, mode).to(P.BF)
    if mutant == "transpose4":
        y[20:24, 36:40] = y[20:24, 36:40].t().clone()
    buf, view = P.out_buffer(M, N)
    view.copy_(y)
    if mutant == "leak":  # row M - 1 read for the padded row and stored at row M
        buf.as_strided((1, N), (view.stride(0), 1), M * view.stride(0)).copy_(y[M - 1:M])
    return buf, view


def _probe(name):
    if name == "D":
        x, w = P.dense_sign(40, 256, 256, 1.0, seed=4)
        return x, w, {}, {}
    if name == "H":
        x, w, k0, side = P.one_hot(40, 256, 256)
        return x, w, {}, dict(k0=k0, side=side)
    if name == "Hx":
        x, w, k0, side = P.one_hot(300, 256, 256)
        return x, w, {}, dict(k0=k0, side=side)
    if name == "R":
        x, w = P.rounding(8, 256, 256, P.split_pairs(256, 2))
        return x, w, dict(splits=2), {}
    assert name == "E"  # bias + ReLU on an exact accumulator
    x, w = P.dense_sign(40, 256, 256, 1.0, seed=5)
    return x, w, dict(bias=P.int_vector(256, -64, 64, 8), relu=True), {}


def _want(name, x, w, kw):
    acc = P.expect(x, w)
    return P.exp_bias_relu(acc, kw["bias"]) if name == "E" else P.rbf(acc)


def _verdict(name, mutant):
    x, w, kw, ck = _probe(name)
    buf, view = blocked_gemm(x, w, mutant=mutant, **kw)
    P.check("H" if name == "Hx" else name, view, _want(name, x, w, kw), f"{name} / {mutant}", **ck)
    P.check_sentinel(buf, view, f"{name} / {mutant}")


@pytest.mark.parametrize("name", ["D", "H", "Hx", "R", "E"])
def test_the_emulation_passes_unmutated(name):
    _verdict(name, None)


MUTANTS = [("drop", "D"), ("drop", "H"), ("chunk", "D"), ("chunk", "H"), ("twice", "D"), ("twice", "H"),
           ("swap_x", "D"), ("swap_x", "H"), ("swap_x", "Hx"), ("leak", "D"), ("leak", "H"), ("leak", "R"),
           ("transpose4", "D"), ("transpose4", "H"), ("trunc", "R"), ("half_away", "R"), ("partial_bf16", "R"),
           ("bias_after", "E")]


@pytest.mark.parametrize("mutant,name", MUTANTS)
def test_every_mutant_fails_its_probe(mutant, name):
    with pytest.raises(AssertionError) as info:
        _verdict(name, mutant)
    if name == "H" and mutant == "drop":
        assert "k = 133" in str(info.value), "H names the k that was dropped"


def test_half_up_store_fails_r():
    x, w, kw, _ = _probe("R")
    buf, view = blocked_gemm(x, w, store="half_up", **kw)
    with pytest.raises(AssertionError):
        P.check("R", view, P.rbf(P.expect(x, w)), "R / half_up")
