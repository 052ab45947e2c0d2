"""tests/row_probes.py without a GPU: the float64 answers against independent integer / closed-form
answers where the probes are exact, the tolerance constants against their measurement, and -- the
point of the probes -- that the f32 emulation of each kernel passes every probe unmutated and fails
at least one with ONE injected fault, under the rule the GPU tests use."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_probes as G  # noqa: E402
import row_probes as R  # noqa: E402

from llm_kubernetes_minikube_sharp4dev_amd.ops import reference as ref  # noqa: E402

BF = torch.bfloat16


# ---------------------------------------------------------------- tolerances
def test_tolerance_constants_match_their_measurement():
    got = R.measure_ulps()
    assert set(got) == set(R.MEASURED)
    for kind, m in got.items():
        assert R.MEASURED[kind] == math.ceil(m * 1000 - 1e-9) / 1000, f"{kind}: measured {m}"
        assert R.ULPS[kind] == 2 * R.MEASURED[kind]


def test_rounding_and_the_rule():
    e = torch.tensor([257.0, 259.0, 2.0 ** -133 * 1.5, 2.0 ** -133 * 2.5, 3.39e38, 3.4e38, float("inf"), float("nan")], dtype=torch.float64)
    r = R.to_bf16(e)
    assert r[:6].tolist() == [256.0, 260.0, 2.0 ** -132, 2.0 ** -132, float(torch.tensor(3.39e38).to(BF)), float("inf")]
    assert math.isinf(float(r[6])) and math.isnan(float(r[7]))
    x = torch.arange(-2400, 2401, dtype=torch.float64) / 8  # f32 holds them: no double rounding
    assert torch.equal(R.to_bf16(x), G.round_bf16(x)) and torch.equal(R.to_bf16(x), x.float().to(BF).double())
    # an expected zero, NaN, inf or sentinel must be met exactly; NaN where a number is due fails
    want = torch.tensor([[0.0, float("nan"), float("inf"), R.SENTINEL, 1.0]], dtype=torch.float64)
    good = torch.tensor([[-0.0, float("nan"), float("inf"), R.SENTINEL, 1.0]]).to(BF)
    R.check("gelu", good, want)
    for i, v in enumerate([1e-30, 1.0, 3e38, R.SENTINEL + 128, float("nan")]):
        b = good.clone()
        b[0, i] = v
        with pytest.raises(AssertionError):
            R.check("gelu", b, want)
    assert float(R.ulp_f32(torch.tensor([1.0], dtype=torch.float64))) == 2.0 ** -23


# ---------------------------------------------------------------- norms: exact answers
def test_row_cfg_covers_every_h_with_an_arm():
    arms = {(1, 1), (1, 2), (2, 1), (4, 1), (4, 2), (4, 3), (4, 4), (4, 5), (4, 6), (4, 7), (4, 8)}
    for H in range(8, 16385, 8):
        assert R.row_cfg(H) in arms, H
    # the shape of every H the missing arm did not refuse is what it always was
    old = lambda nv: 4 if nv >= 256 else (2 if nv >= 128 else 1)  # noqa: E731
    for H in range(8, 16385, 8):
        if not 129 <= H // 8 <= 255:
            assert R.row_cfg(H)[0] == old(H // 8)
    assert R.row_cfg(16392)[1] == 9
    for H in R.NORM_H:
        nvec, nw = H // 8, R.row_cfg(H)[0]
        sv = R.spike_vectors(H)
        assert {0, 1, nvec - 2, nvec - 1} & set(range(nvec)) <= set(sv)
        if H <= 2048:
            assert sv == list(range(nvec))
        for m in range(64 * nw, nvec, 64 * nw):
            assert m in sv and m - 1 in sv


@pytest.mark.parametrize("H", [8, 520, 1536, 4104])
def test_norm_answers_against_closed_forms(H):
    w, b = R.gamma(H), R.beta(H)
    assert H < 16 or (w.double().unique().numel() > 8 and not torch.equal(w[:8], w[8:16]))
    x, ns = R.norm_rows(H)
    sp, col = R.spikes(H)
    want = R.rms64(x, w)
    r = torch.arange(ns)
    closed = 16.0 / math.sqrt(256.0 / H + R.NORM_EPS) * w.double()[col]
    assert torch.allclose(want[r, col], closed, rtol=1e-14, atol=0)
    mask = torch.ones_like(want[:ns], dtype=torch.bool)
    mask[r, col] = False
    assert bool((want[:ns][mask] == 0).all()) and bool((want[ns + 3] == 0).all()), "spike rows and the zero row"
    tiny = want[ns + 4] / w.double()
    assert torch.allclose(tiny[w != 0].abs(), torch.full_like(tiny[w != 0], 2.0 ** -10 / math.sqrt(2.0 ** -20 + R.NORM_EPS)), rtol=1e-13)
    assert 2.0 ** -20 < R.NORM_EPS / 10, "eps dominates the tiny row"
    # the residual sums hold ties and tell the rounding modes apart; int64 arithmetic on halves
    xr, res = R.resid_rows(H)
    s2 = (2 * xr.float()).long() + (2 * res.float()).long()
    assert torch.equal(s2.double() / 2, xr.double() + res.double())
    G.assert_rounding_separates(xr.double() + res.double())
    assert torch.equal(R.add64(xr, res), G.round_bf16(xr.double() + res.double()))
    assert bool(((s2 % 4).abs() == 2).any()), "exact ties: odd integers above 256"
    # LayerNorm: zero variance gives the bias bit for bit (0 without one); spikes in closed form
    xl, nl = R.ln_rows(H)
    lw, _ = R.ln64(xl, w, b)
    l0, _ = R.ln64(xl, w, None)
    for row in (nl, nl + 1):
        assert torch.equal(lw[row], b.double()) and bool((l0[row] == 0).all())
    m, var = 16.0 / H, 256.0 / H - (16.0 / H) ** 2
    assert torch.allclose(l0[torch.arange(nl), col], (16 - m) / math.sqrt(var + R.NORM_EPS) * w.double()[col], rtol=1e-12)
    assert float(xl[nl + 2].double().mean()) == 256 and float(xl[nl + 3].double().mean()) == 256
    tok, pos, typ = R.embed_tables(H)
    ids, pid, yid = R.embed_ids()
    e = R.embed_sum(ids, pid, yid, tok, pos, typ)
    assert torch.equal(e, (tok.long()[ids.long()] + pos.long()[pid.long()] + typ.long()[yid.long()]).double())
    assert bool((e[1] == 2).all()) and 0 in ids.tolist() and 15 in ids.tolist()
    assert torch.equal(R.embed_sum(ids, None, None, tok, None, typ), (tok.long()[ids.long()] + typ.long()[0]).double())


# ---------------------------------------------------------------- norms: sensitivity
def _norm_verdict(op, H, mutant, c=0):
    w, b = R.gamma(H), R.beta(H)
    xr, res = R.resid_rows(H)
    if op == "rms":
        x, _ = R.norm_rows(H)
        for v in (x, R.add64(xr, res)):
            R.check("rms", R.emu_rms(v, w, mutant=mutant, c=c), R.rms64(v, w), f"rms H{H} {mutant}")
    else:
        x, _ = R.ln_rows(H)
        for v in (x, R.add64(xr, res)):
            for bb in (b, None):
                want, fl = R.ln64(v, w, bb)
                R.check("ln", R.emu_ln(v, w, bb, mutant=mutant, c=c), want, f"ln H{H} {mutant}", floor=fl)


@pytest.mark.parametrize("op", ["rms", "ln"])
@pytest.mark.parametrize("H", [8, 520, 1032, 2048, 8200])
def test_norm_emulations_pass_unmutated(op, H):
    _norm_verdict(op, H, None)


NORM_MUTANTS = ["drop", "twice", "padded_width", "no_eps", "eps_outside", "weight_shift"]


@pytest.mark.parametrize("op,mutant", [(o, m) for o in ("rms", "ln") for m in NORM_MUTANTS] + [("ln", "var_e2")])
@pytest.mark.parametrize("H,c", [(520, 64), (4104, 511)])
def test_every_norm_mutant_fails(op, mutant, H, c):
    assert c in R.spike_vectors(H) and R.row_cfg(H)[0] * 64 * R.row_cfg(H)[1] * 8 != H
    with pytest.raises(AssertionError):
        _norm_verdict(op, H, mutant, c)


# ---------------------------------------------------------------- RoPE + KV write
ROPE_CPU = [(neox, wki, D) for neox in (True, False) for wki in (True, False) for D in (32, 96)]


def _rope_verdict(neox, wki, D, mutant, table="synth", T=5, Hq=4, Hkv=2, BS=8, NB=3):
    cs = R.synth_table(R.ROPE_MAX_POS, D) if table == "synth" else R.real_table(D)
    pos = torch.tensor([R.ROPE_POS[(t + 1) % 4] if table == "real" else (7 * t + 2) % R.ROPE_MAX_POS for t in range(T)], dtype=torch.int32)
    buf, qkv = R.qkv_rows(T, Hq, Hkv, D)
    slots = R.slot_list(T, NB, BS)
    want = R.rope_want(qkv.clone(), buf, pos, cs, Hq, Hkv, D, neox, wki, NB, BS, slots)
    kc = torch.full((NB, Hkv, BS, D), R.SENTINEL, dtype=BF)
    vc = kc.clone()
    R.emu_rope_kv(qkv, pos, cs, Hq, Hkv, D, kc, vc, slots, neox, wki, mutant)
    what = f"rope neox {neox} wki {wki} D{D} {mutant}"
    if table == "synth":
        R.check("E", buf, R.exact_bf16(want["row"]), what + ": row")
        R.check("E", kc, R.exact_bf16(want["kc"]), what + ": k cache")
    else:
        R.check("rope", buf, want["row"], what + ": row", floor=want["row_floor"])
        R.check("rope", kc, want["kc"], what + ": k cache", floor=want["kc_floor"])
    R.check("E", vc, R.exact_bf16(want["vc"]), what + ": v cache")


@pytest.mark.parametrize("neox,wki,D", ROPE_CPU)
@pytest.mark.parametrize("table", ["synth", "real"])
def test_rope_emulation_passes_unmutated(neox, wki, D, table):
    _rope_verdict(neox, wki, D, None, table)


ROPE_MUTANTS = ["swap_cs", "sin_sign", "pairing", "freq_shift", "neighbour_pos", "k_unrotated", "v_rotated", "blk_off",
                "cache_layout", "pad_to_slot0", "k_inplace_always"]


@pytest.mark.parametrize("mutant", ROPE_MUTANTS)
def test_every_rope_mutant_fails(mutant):
    failed = 0
    for neox, wki, D in ROPE_CPU:
        try:
            _rope_verdict(neox, wki, D, mutant)
        except AssertionError:
            failed += 1
    want = len(ROPE_CPU) // 2 if mutant == "k_inplace_always" else len(ROPE_CPU)  # shows only with write_k_inplace off
    assert failed == want, f"{mutant}: {failed} of {len(ROPE_CPU)} probes failed"


def test_rope_answers_are_exact_and_independent():
    D, T, Hq, Hkv = 32, 5, 5, 1
    cs = R.synth_table(R.ROPE_MAX_POS, D)
    assert set(cs.unique().tolist()) == set(R.TABLE_VALS)
    assert not torch.equal(cs[:, : D // 2], cs[:, D // 2:]) and not torch.equal(cs[1], cs[2])
    assert torch.equal(R.real_table(D), ref.rope_cos_sin(R.ROPE_MAX_POS, D, theta=R.ROPE_THETA))
    pos = torch.tensor([3, 0, 7, 63, 1], dtype=torch.int32)
    buf, qkv = R.qkv_rows(T, Hq, Hkv, D)
    assert float(qkv.double().abs().max()) <= 32 and bool((buf[:, -8:] == R.SENTINEL).all())
    x = qkv.double()
    for neox in (True, False):
        want = R.rope_want(qkv, buf, pos, cs, Hq, Hkv, D, neox, True)["row"][:T, : (Hq + 2 * Hkv) * D]
        R.exact_bf16(want)  # every result is a bf16 value
        h = x[:, : (Hq + Hkv) * D].reshape(T, Hq + Hkv, D)
        z = torch.complex(h[..., : D // 2], h[..., D // 2:]) if neox else torch.complex(h[..., 0::2], h[..., 1::2])
        rot = z * torch.complex(cs[pos.long()][:, None, : D // 2].double(), cs[pos.long()][:, None, D // 2:].double())
        y = torch.cat([rot.real, rot.imag], -1) if neox else torch.stack([rot.real, rot.imag], -1).flatten(-2)
        assert torch.equal(want[:, : (Hq + Hkv) * D], y.reshape(T, -1)), "the rotation as a complex product"
        assert torch.equal(want[:, (Hq + Hkv) * D:], x[:, (Hq + Hkv) * D:]), "v stays"
        real = R.rope_want(qkv, buf, torch.zeros(T, dtype=torch.int32), R.real_table(D), Hq, Hkv, D, neox, True)
        assert torch.equal(real["row"][:T, : x.shape[1]], x), "position 0 of a real table returns the input"
    for T_, NB, BS in ((1, 3, 8), (3, 8, 1), (5, 3, 128), (5, 3, 16)):
        s = R.slot_list(T_, NB, BS)
        assert NB * BS - 1 in s and (T_ < 2 or 0 in s) and (T_ < 3 or -1 in s)
        assert T_ == 1 or s != sorted(s), "not ascending"
        assert all(-1 <= v < NB * BS for v in s)
    k = torch.arange(2 * 3 * 8, dtype=torch.float32).reshape(2, 3, 8).to(BF)
    kc, vc = R.kv_want(k, -k, [9, -1], 2, 8)
    assert torch.equal(kc[1, :, 1], k[0]) and torch.equal(vc[1, :, 1], -k[0]) and int((kc != R.SENTINEL).sum()) == 24
    c2, v2 = torch.full_like(kc, R.SENTINEL), torch.full_like(kc, R.SENTINEL)
    ref.kv_write(k, -k, c2, v2, torch.tensor([9, -1], dtype=torch.int32))
    assert torch.equal(c2, kc) and torch.equal(v2, vc)


# ---------------------------------------------------------------- activations
def test_activation_inputs_and_answers():
    allb = R.all_bf16()
    assert allb.view(torch.int16).unique().numel() == 65536
    a = R.act_input(8192, 8)
    assert torch.equal(a.flatten().view(torch.int16), allb.view(torch.int16))
    x = R.silu_input(65540, 8)
    g, u = x[:, :8].flatten(), x[:, 8:].flatten()
    assert torch.equal(g[:65536].view(torch.int16), allb.view(torch.int16)) and bool((u[:65536] == 1).all())
    seen = {(int(p), float(v)) for p, v in zip(g[65536:].view(torch.int16).tolist()[:: 7], u[65536:].tolist()[:: 7])}
    assert {v for _, v in seen} == set(R.UPS)
    b = R.act_bias(8)
    fin = a.double()[torch.isfinite(a.double()).all(1) & (a.double().abs() < 1e30).all(1) & (a.double().abs() > 1e-30).all(1)]
    G.assert_rounding_separates(fin + b.double()[None, :])  # x + bias holds exact ties
    # the float64 formulas at the edges: NaN-ness and infinities
    e = torch.tensor([[float("inf"), float("-inf"), float("nan"), -0.0, -1e30, 1e30, -100.0, 2.0 ** -130]]).to(BF)
    for kind in (0, 1):
        w, _, keep = R.act64(e, None, kind)
        assert math.isinf(float(w[0, 0])) and math.isnan(float(w[0, 1])) and math.isnan(float(w[0, 2])) and bool(keep.all())
        assert w[0, 3:7].tolist() == [0.0, 0.0, float(e[0, 5]), 0.0] and float(w[0, 7]) == 2.0 ** -131
    w, _, keep = R.act64(e, None, 2)
    assert keep[0].tolist() == [True, True, False] + [True] * 5 and float(w[0, 0]) == float("inf") and float(w[0, 1]) == 0
    s, fl = R.silu_mul64(torch.cat([e, torch.full_like(e, 3.0)], 1))
    assert math.isinf(float(s[0, 0])) and math.isnan(float(s[0, 1])) and math.isnan(float(s[0, 2])) and float(s[0, 4]) == 0
    assert float(fl[0, 7]) == 3 * R.SUBNORMAL and float(fl[0, 6]) == 3 * R.SILU_TINY
    big = torch.tensor([[3.0e38, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]]).to(BF)
    assert math.isinf(float(R.silu_mul64(torch.cat([big, torch.full_like(big, 3.0)], 1))[0][0, 0])), "the store overflows"


def _act_verdict(op, bias, mutant):
    if op == "silu":
        x = R.silu_input(8192 + 4096, 8)
        want, fl = R.silu_mul64(x)
        R.check("silu", R.emu_silu_mul(x, mutant), want, f"silu_mul {mutant}", floor=fl)
        return
    kind = {"gelu": 0, "gelu_tanh": 1, "relu": 2}[op]
    a = R.act_input(8192, 8)
    b = R.act_bias(8) if bias else None
    want, fl, keep = R.act64(a, b, kind)
    got = R.emu_act(a, b, kind, mutant)
    if kind == 2:
        R.check("E", torch.where(keep, got.double(), torch.zeros_like(want)), want, f"relu {mutant}")
    else:
        R.check(op, got, want, f"{op} bias {bias} {mutant}", floor=fl)


@pytest.mark.parametrize("op,bias", [("silu", False)] + [(o, b) for o in ("gelu", "gelu_tanh", "relu") for b in (False, True)])
def test_activation_emulations_pass_unmutated(op, bias):
    _act_verdict(op, bias, None)


@pytest.mark.parametrize("op,bias,mutant", [("gelu", False, "tanh_for_erf"), ("gelu", True, "bias_after"), ("gelu_tanh", True, "bias_after"),
                                            ("relu", True, "bias_after"), ("relu", True, "trunc")])
def test_every_activation_mutant_fails(op, bias, mutant):
    """A truncating f2bf shows where the answer is exact: the ties of x + bias under ReLU.  After the
    GELUs and in silu_mul it moves an inexact value by less than one ulp, inside their bounds."""
    with pytest.raises(AssertionError):
        _act_verdict(op, bias, mutant)


def test_tanh_gelu_differs_from_erf_gelu_at_249_values():
    x = R.all_bf16().double()
    x = x[torch.isfinite(x)]
    d = (R.gelu_tanh64(x) - G.gelu64(x)).abs()
    assert int((d > 2 * R.ulp_bf(G.gelu64(x))).sum()) == 249


# ---------------------------------------------------------------- pooling, row norms
@pytest.mark.parametrize("H", [8, 1032])
def test_pool_answers_emulation_and_reference(H):
    _, hid, cu = R.pool_hidden(H)
    assert hid.stride(0) == H + 8 and cu.tolist() == [0, 3, 3, 4, 44, 44, 46]
    h = hid.double()
    assert torch.equal(h, h.round()) and bool((h[44:] == 0).all())
    for mode in (0, 1):
        for nrm in (True, False):
            want = R.pool64(hid, cu, mode, nrm)
            assert bool(torch.isfinite(want).all()) and bool((want[[1, 4, 5]] == 0).all()), "empty and all-zero sequences"
            if not nrm:
                n = torch.tensor([3, 1, 1, 40, 1, 2], dtype=torch.float64)[:, None]
                ints = torch.stack([h[a:b].sum(0) if mode == 0 else (h[a] if b > a else torch.zeros(H, dtype=torch.float64))
                                    for a, b in zip(cu[:-1].tolist(), cu[1:].tolist())])
                assert torch.equal(want * (n if mode == 0 else 1), ints) or torch.allclose(want * n, ints, rtol=1e-15, atol=0)
            else:
                nz = want.pow(2).sum(1)
                assert torch.allclose(nz[[0, 2, 3]], torch.ones(3, dtype=torch.float64), rtol=1e-14)
            R.check("pool", R.emu_pool(hid, cu, mode, nrm), want, f"pool H{H} mode {mode} normalize {nrm}")
            R.check("pool", R.emu_pool(hid, cu, mode, nrm).to(BF), want, "bf16 destination", floor=R.pool_bf16_floor(want))
            # the CPU fallback of ops.pool_normalize: zeros for empty sequences, like the kernel
            got = ref.pool_normalize(hid, cu, mode, nrm)
            assert got.shape == want.shape and bool((got[[1, 4]] == 0).all())
            R.check("pool", got, want, "ops.reference.pool_normalize")


@pytest.mark.parametrize("mutant,mode", [("n_plus_1", 0), ("div_h", 0), ("cls_last", 1), ("next_seq", 0), ("no_clamp", 0), ("no_clamp", 1)])
def test_every_pool_mutant_fails(mutant, mode):
    _, hid, cu = R.pool_hidden(1032)
    for nrm in ((True,) if mutant == "no_clamp" else (False,)):
        with pytest.raises(AssertionError):
            R.check("pool", R.emu_pool(hid, cu, mode, nrm, mutant), R.pool64(hid, cu, mode, nrm), mutant)


@pytest.mark.parametrize("D", [8, 512, 520, 1032])
def test_square_rows_are_perfect_squares(D):
    x, nrm = R.square_rows(9, D)
    ss = x.long().pow(2).sum(1)
    assert torch.equal(ss.double(), nrm * nrm) and int(ss.max()) < 2 ** 24
    assert bool((x[:, -8:] != 0).any()) and bool((x[:, :8] != 0).any()), "the first and the last vector count"
    R.check("rownorm", ref.row_norms(x), nrm, "ops.reference.row_norms")
    with pytest.raises(AssertionError):
        R.check("rownorm", x[:, 8:].float().norm(dim=-1), nrm, "a vector dropped")


# ---------------------------------------------------------------- argmax key
def _old_argmax_key(logits, vocab_lo=0):
    """The key without the signed-zero canonicalisation: +0.0 orders above -0.0."""
    x = logits.float()
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
    idx = x.argmax(-1)
    best = x.gather(1, idx[:, None]).squeeze(1)
    fb = best.view(torch.int32).long() & 0xFFFFFFFF
    u = torch.where(fb >= 0x80000000, (~fb) & 0xFFFFFFFF, fb | 0x80000000)
    hi = (u ^ 0x80000000) - ((u ^ 0x80000000) >= 0x80000000).long() * (1 << 32)
    return hi * (1 << 32) + ((~(idx + vocab_lo)) & 0xFFFFFFFF)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [50, 1003])
def test_argmax_key_rows(dtype, V):
    logits, names = R.key_rows(V, dtype)
    want = R.key_want(logits)
    assert want[names.index("all -inf")] == 0 and want[names.index("-0.0 at id 1, +0.0 later")] == 1
    b = R.shard_bounds(V, 3)
    assert want[names.index("a tie across shards")] == b[1] - 1 and want[names.index("the maximum in the last column")] == V - 1
    for W in (1, 2, 3):
        got = R.key_ids(logits, W, ref.argmax_key, ref.keys_to_ids)
        assert got.tolist() == want.tolist(), [n for n, g, w in zip(names, got.tolist(), want.tolist()) if g != w]
    old = R.key_ids(logits, 3, _old_argmax_key, ref.keys_to_ids).tolist()
    wrong = {n for n, g, w in zip(names, old, want.tolist()) if g != w}
    assert wrong == {"-0.0 in shard 0, +0.0 later", "-0.0 at id 1, +0.0 later"}, wrong


def test_the_issue_example_of_the_signed_zero_key():
    row = torch.tensor([[-1, -0.0, -2, -3, -5, 0.0, -1, -7]])
    keys = lambda f: torch.stack([f(row[:, :4], 0), f(row[:, 4:], 4)])  # noqa: E731
    assert int(row.argmax()) == 1
    assert ref.keys_to_ids(keys(_old_argmax_key)).tolist() == [5]
    assert ref.keys_to_ids(keys(ref.argmax_key)).tolist() == [1]
