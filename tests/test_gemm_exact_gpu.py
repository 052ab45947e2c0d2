"""The linear-layer kernels against the structured probes of tests/gemm_probes.py, whose float64
answers pin every single product, the rounding of the store and each epilogue: the decode GEMV
(csrc/gemv_decode.hip), the fragment-load and weight-streaming decode GEMMs (csrc/skinny_gemm.hip),
the prefill GEMMs (csrc/gemm.hip, csrc/gemm1w.hip) and the routing of ops.linear between them.
tests/test_gemm_probes_cpu.py shows what these comparisons reject."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_probes as P  # noqa: E402

from llm_kubernetes_minikube_sharp4dev_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


class Checks:
    """Comparisons counted on the device, read back once: finish() raises for the first failure,
    with the indices (and, for H, the k) from gemm_probes.check()."""

    def __init__(self):
        self.items = []

    def add(self, kind, got, want, what, buf=None, floor=None, **kw):
        assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
        if kind in P.ULPS:
            n = (P.excess_ulps(got, want, floor) > P.ULPS[kind]).sum()
        else:
            assert got.dtype == want.dtype, what
            n = (got != want).sum()
        if buf is not None:  # whatever is not the sentinel lies inside the result
            n = n + ((buf != P.SENTINEL).sum() - (got != P.SENTINEL).sum())
        self.items.append((n, kind, got, want, what, buf, floor, kw))

    def finish(self):
        if not self.items:
            return
        counts = torch.stack([it[0] for it in self.items]).tolist()
        items, self.items = self.items, []
        for c, (_, kind, got, want, what, buf, floor, kw) in zip(counts, items):
            if c:
                P.check(kind, got, want, what, floor=floor, **kw)
                if buf is not None:
                    P.check_sentinel(buf, got, what)
                raise AssertionError(f"{what}: {c} elements off")


@functools.lru_cache(maxsize=6)
def _dense(M, N, K, density=1.0, seed=0):
    """D on the device with its float64 accumulator; density 1: the 5 % cap, else the 192 cap."""
    x, w = P.dense_sign(M, N, K, density, seed, DEV)
    acc = P.expect(x, w)
    if density >= 1.0 and K > P.SENS_CAP:
        P.assert_sensitive(acc)
    else:
        P.assert_acc_cap(acc)
    return x, w, acc


def _low(M, N, K, seed=1):
    return _dense(M, N, K, P.epi_density(K), seed)


# ================================================================ GEMV (hip.gemv_decode, no gamma)
GEMV_K = [2048, 3584, 4096, 6144, 7168, 8192, 14336]
GEMV_N = [2, 6, 10, 256, 1030]


def _gemv_knobs(hip):
    hip.gemv_set_wgs(ops.GEMV_WGS)
    hip.gemv_set_ksplit(ops.GEMV_KSPLIT)


@pytest.mark.parametrize("K", GEMV_K)
def test_gemv_dense_and_mode_epilogues(hip, K):
    """D through modes 0 (plain), 1 (res += in place, inside a sentinel-filled buffer) and 2
    (SwiGLU on small accumulators): U = 4 / 7 / 8, one, an odd and an even number of U-blocks, both
    K-split arms, fewer pairs than a workgroup round (N 2, 6, 10) and grid-stride rounds (1 and 3
    workgroups)."""
    NM = max(GEMV_N)
    x, w, acc = _dense(2, NM, K, 1.0)
    xl, wl, accl = _low(2, NM, K)
    res0 = P.int_matrix(2, NM, -32, 32, K, DEV)
    want0 = P.rbf(acc)
    want1, _ = P.exp_resid(acc, res0)
    want2 = {N: (P.swiglu64(accl[:, : N // 2], accl[:, N // 2:N]), P.swiglu_floor(accl[:, N // 2:N])) for N in GEMV_N}
    ck = Checks()
    try:
        for wgs in (0, 1, 3):
            hip.gemv_set_wgs(wgs)
            for ksplit in (True, False):
                hip.gemv_set_ksplit(ksplit)
                for M in (1, 2):
                    for N in GEMV_N:
                        what = f"gemv K{K} N{N} M{M} wgs {wgs} ksplit {ksplit}"
                        for mode in range(3):
                            assert hip.gemv_supported(M, N, K, mode), what
                        ck.add("D", hip.gemv_decode(0, x[:M], w[:N]), want0[:M, :N], what + " mode 0")
                        buf, res = P.out_buffer(M, N, DEV)
                        res.copy_(res0[:M, :N])
                        out = hip.gemv_decode(1, x[:M], w[:N], res=res)
                        assert out.data_ptr() == res.data_ptr()
                        ck.add("E", res, want1[:M, :N], what + " mode 1", buf=buf)
                        y = hip.gemv_decode(2, xl[:M], wl[:N])
                        ck.add("swiglu", y, want2[N][0][:M], what + " mode 2", floor=want2[N][1][:M])
                ck.finish()
    finally:
        _gemv_knobs(hip)


@pytest.mark.parametrize("K", GEMV_K)
def test_gemv_one_hot(hip, K):
    """H, one-hot on W: N = K up to 4096, above that 2048 rows shifted until every k was selected."""
    N = K if K <= 4096 else 2048
    ck = Checks()
    try:
        for ksplit in (True, False):
            hip.gemv_set_ksplit(ksplit)
            for wgs in (0, 3):
                hip.gemv_set_wgs(wgs)
                for shift in P.hot_shifts(N, K):
                    x, w, k0, side = P.one_hot(2, N, K, shift, DEV)
                    want = P.rbf(P.one_hot_expect(x, w, k0, side))
                    for M in (1, 2):
                        assert hip.gemv_supported(M, N, K, 0)
                        ck.add("H", hip.gemv_decode(0, x[:M], w), want[:M],
                               f"gemv H K{K} M{M} shift {shift} wgs {wgs} ksplit {ksplit}", k0=k0, side=side)
                ck.finish()
    finally:
        _gemv_knobs(hip)


@pytest.mark.parametrize("K", GEMV_K)
def test_gemv_rounding(hip, K):
    """R: one round-to-nearest-even at the store, the two terms in different K halves (the two
    waves of the K-split) and different U-blocks."""
    N = 256
    pairs = P.split_pairs(K, 2)
    ck = Checks()
    try:
        for start in range(len(pairs)):
            x, w = P.rounding(2, N, K, pairs, start, DEV)
            e = P.expect(x, w)
            if len(pairs[start]) == 2:
                P.assert_rounding_separates(e[:1])
            for ksplit in (True, False):
                hip.gemv_set_ksplit(ksplit)
                for M in (1, 2):
                    ck.add("R", hip.gemv_decode(0, x[:M], w), P.rbf(e[:M]), f"gemv R K{K} M{M} start {start} ksplit {ksplit}")
        ck.finish()
    finally:
        _gemv_knobs(hip)


def _qkv_checks(ck, what, out, kc, vc, acc, pos, slots, cs, Hq, Hkv, D, neox, k_rotated_in_row):
    """A packed QKV row after RoPE and the paged-KV write, from the exact accumulator: q rotated, k
    rotated in the cache (and in the row if k_rotated_in_row), v copied; position 0 bit for bit, other
    positions to the RoPE tolerance; cache rows of no slot untouched (the caches start as SENTINEL)."""
    qkv = P.rbf(acc).double()
    BS = kc.shape[2]
    row_want, row_floor = P.rope_expect(qkv, pos, cs, Hq, Hkv, D, neox, k_rotated_in_row)
    cache_want, cache_floor = P.rope_expect(qkv, pos, cs, Hq, Hkv, D, neox, True)
    kcols = slice(Hq * D, (Hq + Hkv) * D)
    vcols = slice((Hq + Hkv) * D, (Hq + 2 * Hkv) * D)
    zero = pos == 0
    sel = slots >= 0
    blk, off = (slots[sel] // BS).long(), (slots[sel] % BS).long()
    gk = kc[blk, :, off, :].reshape(-1, Hkv * D)
    gv = vc[blk, :, off, :].reshape(-1, Hkv * D)
    for z, name in ((zero, "position 0"), (~zero, "rotated")):
        if bool(z.any()):
            if name == "position 0":
                ck.add("E", out[z], row_want[z].to(BF), f"{what}: row, {name}")
            else:
                ck.add("rope", out[z], row_want[z], f"{what}: row, {name}", floor=row_floor[z])
        zs = z[sel]
        if bool(zs.any()):
            if name == "position 0":
                ck.add("E", gk[zs], cache_want[sel][zs][:, kcols].to(BF), f"{what}: k cache, {name}")
            else:
                ck.add("rope", gk[zs], cache_want[sel][zs][:, kcols], f"{what}: k cache, {name}",
                       floor=cache_floor[sel][zs][:, kcols])
    if bool(sel.any()):
        ck.add("E", gv, qkv[sel][:, vcols].to(BF), f"{what}: v cache")
    for c, name in ((kc, "k"), (vc, "v")):
        rest = c.clone()
        rest[blk, :, off, :] = P.SENTINEL
        ck.add("E", rest.view(-1, D), torch.full_like(rest, P.SENTINEL).view(-1, D), f"{what}: {name} cache outside the slots")


@pytest.mark.parametrize("neox", [True, False])
def test_gemv_rope_kv(hip, neox):
    """Mode 3 on small exact accumulators at Hq 2, Hkv 1, D 64: position 0 rotates by (1, 0) and is
    bit-exact, position 37 within the RoPE tolerance of the float64 rotation; one slot is -1."""
    Hq, Hkv, D, BS = 2, 1, 64, 16
    N = (Hq + 2 * Hkv) * D
    cs = P.rope_table(64, D, DEV)
    ck = Checks()
    try:
        for K in GEMV_K:
            x, w, acc = _low(2, N, K, seed=3)
            for ksplit in (True, False):
                hip.gemv_set_ksplit(ksplit)
                for M, pos, slots in ((2, [0, 37], [5 * BS + 3, -1]), (2, [37, 0], [2 * BS + 15, -1]), (1, [37], [7]),
                                      (1, [0], [BS])):
                    assert hip.gemv_supported(M, N, K, 3)
                    pos_t = torch.tensor(pos, dtype=torch.int32, device=DEV)
                    slots_t = torch.tensor(slots, dtype=torch.int32, device=DEV)
                    kc = torch.full((8, Hkv, BS, D), P.SENTINEL, dtype=BF, device=DEV)
                    vc = kc.clone()
                    out = hip.gemv_decode(3, x[:M], w, None, 1e-5, None, pos_t, cs, Hq, Hkv, D, kc, vc, slots_t, neox)
                    _qkv_checks(ck, f"gemv mode 3 K{K} neox {neox} pos {pos} ksplit {ksplit}", out, kc, vc, acc[:M], pos_t,
                                slots_t, cs, Hq, Hkv, D, neox, False)
            ck.finish()
    finally:
        _gemv_knobs(hip)


# ================================================================ skinny (hip.skinny_linear)
DECODE_M = [1, 15, 16, 17, 32, 33, 64, 65, 128, 129, 256]
SKINNY_SK = [(S, 256 * S * j) for S in (1, 2, 4, 8) for j in (1, 2, 3)]


@pytest.mark.parametrize("M", DECODE_M)
def test_skinny_dense(hip, M):
    """D with SwiGLU off (bit-exact) and on (small accumulators), every explicit split at one, two
    and three K-steps per wave, into a sentinel-filled buffer with ldo > N."""
    ck = Checks()
    for N in (64, 192):
        for S, K in SKINNY_SK:
            what = f"skinny M{M} N{N} K{K} S{S}"
            x, w, acc = _dense(M, N, K, 1.0)
            buf, out = P.out_buffer(M, N, DEV)
            hip.skinny_linear(x, w, False, S, out)
            ck.add("D", out, P.rbf(acc), what, buf=buf)
            x, w, acc = _low(M, N, K)
            g, u = acc[:, : N // 2], acc[:, N // 2:]
            buf, out = P.out_buffer(M, N // 2, DEV)
            hip.skinny_linear(x, w, True, S, out)
            ck.add("swiglu", out, P.swiglu64(g, u), what + " swiglu", buf=buf, floor=P.swiglu_floor(u))
        ck.finish()


@pytest.mark.parametrize("M", DECODE_M)
def test_skinny_one_hot(hip, M):
    """H: every k of every split and wave range selected once (shifted launches)."""
    ck = Checks()
    for N in (64, 192):
        for S, K in SKINNY_SK:
            for shift in P.hot_shifts(max(M, N), K):
                x, w, k0, side = P.one_hot(M, N, K, shift, DEV)
                buf, out = P.out_buffer(M, N, DEV)
                hip.skinny_linear(x, w, False, S, out)
                ck.add("H", out, P.rbf(P.one_hot_expect(x, w, k0, side)), f"skinny H M{M} N{N} K{K} S{S} shift {shift}",
                       buf=buf, k0=k0, side=side)
            ck.finish()


@pytest.mark.parametrize("M", DECODE_M)
def test_skinny_rounding(hip, M):
    """R over the 4 S wave ranges of K: the two (three) terms meet in the LDS cross-wave sum and,
    S > 1, in the slab reduce."""
    ck = Checks()
    for N in (64, 192):
        for S, K in SKINNY_SK:
            pairs = P.split_pairs(K, 4 * S)
            for start in range(0, len(pairs), M):
                x, w = P.rounding(M, N, K, pairs, start, DEV)
                e = P.expect(x, w)
                buf, out = P.out_buffer(M, N, DEV)
                hip.skinny_linear(x, w, False, S, out)
                ck.add("R", out, P.rbf(e), f"skinny R M{M} N{N} K{K} S{S} start {start}", buf=buf)
        ck.finish()


# ================================================================ weight-streaming (hip.ws_linear)
WS_M = [1, 16, 17, 64, 65, 128, 129, 192, 193, 255, 256]
WS_NST = range(1, 14)  # K-steps per split: 1 .. past the deepest LDS ring (8 stages; loader waves: 12)
WS_N = 384


def _ws_rots(S):
    """0, the policy default (-1: 5 unsplit, off on split-K grids) and 3."""
    return (0, -1, 3) if S == 1 else (-1, 3)


class _WsKnobs:
    """ws_set_variant / ws_set_rot with every key restored on exit."""

    def __init__(self, hip):
        self.hip, self.keys = hip, set()

    def variant(self, M, N, K, swiglu, v):
        self.keys.add((M, N, K, swiglu))
        self.hip.ws_set_variant(M, N, K, swiglu, v)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for key in self.keys:
            self.hip.ws_set_variant(*key, -1)
        self.hip.ws_set_rot(-1)


@pytest.mark.parametrize("BN", [64, 96, 128])
@pytest.mark.parametrize("M", WS_M)
def test_ws_dense(hip, M, BN):
    """D over K walks shorter than, equal to and longer than the LDS ring (the prologue guards and
    the wait_ahead tail), both kernels, every K-step rotation, S 1 / 2 / 4."""
    ck = Checks()
    with _WsKnobs(hip) as knobs:
        for S in (1, 2, 4):
            for nst in WS_NST:
                K = 64 * S * nst
                x, w, acc = _dense(M, WS_N, K, 1.0)
                want = P.rbf(acc)
                for v in (0, 1):
                    knobs.variant(M, WS_N, K, False, v)
                    for rot in _ws_rots(S):
                        hip.ws_set_rot(rot)
                        buf, out = P.out_buffer(M, WS_N, DEV)
                        hip.ws_linear(x, w, False, BN, S, out)
                        ck.add("D", out, want, f"ws M{M} BN{BN} S{S} nst {nst} variant {v} rot {rot}", buf=buf)
            ck.finish()


@pytest.mark.parametrize("BN", [64, 128])
@pytest.mark.parametrize("M", WS_M)
def test_ws_swiglu(hip, M, BN):
    """The SwiGLU epilogue (in the GEMM, S = 1, and in the slab reduce) on small accumulators."""
    N = 768
    ck = Checks()
    with _WsKnobs(hip) as knobs:
        for S in (1, 2, 4):
            for nst in (1, 2, 3, 9):
                K = 64 * S * nst
                x, w, acc = _low(M, N, K)
                g, u = acc[:, : N // 2], acc[:, N // 2:]
                want, floor = P.swiglu64(g, u), P.swiglu_floor(u)
                for v in (0, 1):
                    knobs.variant(M, N, K, True, v)
                    for rot in _ws_rots(S):
                        hip.ws_set_rot(rot)
                        buf, out = P.out_buffer(M, N // 2, DEV)
                        hip.ws_linear(x, w, True, BN, S, out)
                        ck.add("swiglu", out, want, f"ws swiglu M{M} BN{BN} S{S} nst {nst} variant {v} rot {rot}", buf=buf,
                               floor=floor)
        ck.finish()


@pytest.mark.parametrize("BN", [64, 96, 128])
@pytest.mark.parametrize("M", WS_M)
def test_ws_one_hot_and_rounding(hip, M, BN):
    """H (every k of every short walk) and R (the terms in different splits / K-steps), both kernels."""
    ck = Checks()
    with _WsKnobs(hip) as knobs:
        for S in (1, 2, 4):
            for nst in WS_NST:
                K = 64 * S * nst
                probes = []
                for shift in P.hot_shifts(WS_N, K):
                    x, w, k0, side = P.one_hot(M, WS_N, K, shift, DEV)
                    probes.append(("H", x, w, P.rbf(P.one_hot_expect(x, w, k0, side)), f"shift {shift}", dict(k0=k0, side=side)))
                pairs = P.split_pairs(K, S)
                for start in range(0, len(pairs), M):
                    x, w = P.rounding(M, WS_N, K, pairs, start, DEV)
                    probes.append(("R", x, w, P.rbf(P.expect(x, w)), f"start {start}", {}))
                for v in (0, 1):
                    knobs.variant(M, WS_N, K, False, v)
                    for kind, x, w, want, tag, kw in probes:
                        buf, out = P.out_buffer(M, WS_N, DEV)
                        hip.ws_linear(x, w, False, BN, S, out)
                        ck.add(kind, out, want, f"ws {kind} M{M} BN{BN} S{S} nst {nst} variant {v} {tag}", buf=buf, **kw)
            ck.finish()


@pytest.mark.parametrize("M", [1, 17, 65, 129, 193, 256])
def test_ws_views(hip, M):
    """Output views the 8-byte vector stores cannot take (ldo % 4 != 0, out one and two elements
    off) -- in the GEMM (S = 1) and in the slab reduce -- and x as a column slice of a wider buffer."""
    ck = Checks()
    views = [dict(pad_cols=3), dict(pad_cols=8, offset=1), dict(pad_cols=8, offset=2), dict(pad_cols=5, offset=1)]
    with _WsKnobs(hip) as knobs:
        for BN in (64, 96, 128):
            for S in (1, 2):
                K = 64 * S * 3
                x, w, acc = _dense(M, WS_N, K, 1.0)
                wide = torch.full((M, K + 64), 3.0, dtype=BF, device=DEV)
                xs = wide[:, 32:32 + K]
                xs.copy_(x)
                assert xs.stride(0) == K + 64 and xs.data_ptr() % 16 == 0
                for v in (0, 1):
                    knobs.variant(M, WS_N, K, False, v)
                    for kw in views:
                        buf, out = P.out_buffer(M, WS_N, DEV, **kw)
                        hip.ws_linear(xs, w, False, BN, S, out)
                        ck.add("D", out, P.rbf(acc), f"ws view {kw} M{M} BN{BN} S{S} variant {v}", buf=buf)
                if BN != 96:
                    xl, wl, accl = _low(M, 768, K)
                    g, u = accl[:, :384], accl[:, 384:]
                    for kw in views:
                        buf, out = P.out_buffer(M, 384, DEV, **kw)
                        hip.ws_linear(xl, wl, True, BN, S, out)
                        ck.add("swiglu", out, P.swiglu64(g, u), f"ws swiglu view {kw} M{M} BN{BN} S{S}", buf=buf,
                               floor=P.swiglu_floor(u))
        ck.finish()


@pytest.mark.parametrize("neox", [True, False])
@pytest.mark.parametrize("inplace", [False, True])
def test_ws_rope_kv_tail(hip, neox, inplace):
    """ws_linear_rope_kv with BN = D = 128: the last split workgroup of a head rotates and writes the
    paged KV (tickets) -- twice on one ticket buffer -- and the two-launch path; D on small
    accumulators and H, positions 0 (bit-exact) and 37."""
    Hq, Hkv, D, BS = 2, 1, 128, 16
    N = (Hq + 2 * Hkv) * D
    cs = P.rope_table(64, D, DEV)
    ck = Checks()
    for M in (1, 3, 65, 200):
        pos = torch.tensor([0, 37, 37, 0][:M] + [37 * (i % 2) for i in range(max(0, M - 4))], dtype=torch.int32, device=DEV)
        slots = torch.arange(M, dtype=torch.int32, device=DEV) * 3 + 1
        if M > 1:
            slots[1] = -1
        NB = (3 * M + 1) // BS + 2
        for S in (2, 4, 8):
            K = 64 * S * 2
            xh, wh, k0, side = P.one_hot(M, N, K, 0, DEV)
            for name, x, w, acc in (("D", *_low(M, N, K, seed=5)), ("H", xh, wh, P.one_hot_expect(xh, wh, k0, side))):
                tickets = torch.zeros(Hq + 2 * Hkv, dtype=torch.int32, device=DEV)
                for tk, rep in ((tickets, 0), (tickets, 1), (None, 0)):
                    kc = torch.full((NB, Hkv, BS, D), P.SENTINEL, dtype=BF, device=DEV)
                    vc = kc.clone()
                    out = hip.ws_linear_rope_kv(x, w, pos, cs, Hq, Hkv, D, kc, vc, slots, neox, inplace, 128, S, tk)
                    what = f"ws rope_kv {name} M{M} S{S} neox {neox} inplace {inplace} " + \
                        ("two launches" if tk is None else f"fused, call {rep}")
                    if name == "D":
                        _qkv_checks(ck, what, out, kc, vc, acc, pos, slots, cs, Hq, Hkv, D, neox, inplace)
                    else:  # |acc| up to 250: the rows of position 0 (exact), every v, the untouched cache
                        z = pos == 0
                        ck.add("H", out[z], P.rbf(acc)[z], what + ": row, position 0")
                        ck.add("H", out[:, (Hq + Hkv) * D:], P.rbf(acc)[:, (Hq + Hkv) * D:], what + ": v columns")
                    if tk is not None:
                        ck.add("E", tk.view(1, -1), torch.zeros_like(tk).view(1, -1), what + ": tickets reset")
        ck.finish()


@pytest.mark.parametrize("M,S,BN", P.NORM_CASES)
def test_ws_rmsnorm_tail(hip, M, S, BN):
    """ws_linear_rmsnorm: the residual bit-exact, the normed rows within the measured tolerance of
    the float64 RMSNorm of the new residual, on D (small accumulators) and H; the fused tail twice on
    one ticket buffer, and the two-launch path."""
    ck = Checks()
    for name, x, w, res0, gamma in P.norm_cases(M, S, DEV):
        acc = P.expect(x, w)
        new, _ = P.exp_resid(acc, res0)
        tickets = torch.zeros(4, dtype=torch.int32, device=DEV)
        for tk, rep in ((tickets, 0), (tickets, 1), (None, 0)):
            what = f"ws rmsnorm {name} M{M} S{S} BN{BN} " + ("two launches" if tk is None else f"fused, call {rep}")
            buf, res = P.out_buffer(M, P.NORM_N, DEV)
            res.copy_(res0)
            y = hip.ws_linear_rmsnorm(x, w, res, gamma, P.NORM_EPS, BN, S, tk)
            ck.add("E", res, new, what + ": residual", buf=buf)
            ck.add("norm", y, P.norm64(new, gamma), what + ": normed")
            if tk is not None:
                ck.add("E", tk.view(1, -1), torch.zeros_like(tk).view(1, -1), what + ": tickets reset")
    ck.finish()


# ================================================================ prefill (hip.gemm, hip.gemm_fused)
# (variant, column tile): gemm.hip schedules 0-2, gemm1w.hip 3 / 4 / 5 (256 / 192 / 128-row tiles) and its
# column splits 6 / 7
PREFILL_CFGS = [(0, 256), (1, 256), (2, 256), (0, 192), (1, 192), (2, 192), (3, 256), (4, 256), (5, 256), (6, 256), (7, 256)]
PREFILL_M = [1, 127, 128, 129, 191, 192, 193, 255, 256, 257, 385, 1300]
PREFILL_KT = range(1, 10)
PREFILL_N = 768


def _min_kt(variant):
    return 2 if variant <= 2 else 3  # K-tiles a kernel needs: gemm.hip 2, gemm1w.hip 3 (one K-tile: no kernel)


def _cfgs(hip, M, N, K, epi, splits=1):
    """The configurations that run (M, N, K); a variant must support every K its kernel documents."""
    out = []
    for v, bn in PREFILL_CFGS:
        ok = hip.gemm_supported(M, N, K, epi, bn, splits, v)
        if v <= 5 and splits == 1 and K // 64 >= _min_kt(v) and not (epi in (1, 6) and bn == 192):
            assert ok, f"variant {v} bn {bn} rejects M{M} N{N} K{K} epi {epi}"
        if ok:
            out.append((v, bn))
    return out


@pytest.mark.parametrize("M", PREFILL_M)
def test_prefill_dense_one_hot_rounding(hip, M):
    """D, H and R at 1 to 9 K-tiles through every variant and column tile, M tails on both sides of
    the 128 / 192 / 256-row tiles, into a sentinel-filled buffer with ldo > N."""
    N = PREFILL_N
    ck = Checks()
    for kt in PREFILL_KT:
        K = 64 * kt
        x, w, acc = _dense(M, N, K, 1.0)
        probes = [("D", x, w, P.rbf(acc), {})]
        for shift in P.hot_shifts(max(M, N), K):
            xh, wh, k0, side = P.one_hot(M, N, K, shift, DEV)
            probes.append(("H", xh, wh, P.rbf(P.one_hot_expect(xh, wh, k0, side)), dict(k0=k0, side=side)))
        pairs = P.split_pairs(K, 1)
        for start in range(0, len(pairs), M):
            xr, wr = P.rounding(M, N, K, pairs, start, DEV)
            probes.append(("R", xr, wr, P.rbf(P.expect(xr, wr)), {}))
        cfgs = _cfgs(hip, M, N, K, 0)
        assert len(cfgs) >= (0 if kt < 2 else 6 if kt < 3 else 9)
        for v, bn in cfgs:
            for kind, px, pw, want, kw in probes:
                buf, out = P.out_buffer(M, N, DEV)
                hip.gemm(px, pw, None, 0, bn, out, v)
                ck.add(kind, out, want, f"gemm {kind} M{M} K{K} variant {v} bn {bn}", buf=buf, **kw)
        ck.finish()


def _epilogue_case(hip, ck, M, N, K, epi, v, bn, splits, x, w, acc, tag=""):
    what = f"gemm epi {epi} M{M} N{N} K{K} variant {v} bn {bn} splits {splits}{tag}"
    if epi in (2, 3, 4):
        b = P.int_vector(N, -64, 64, N + epi, DEV)
        buf, out = P.out_buffer(M, N, DEV)
        hip.gemm(x, w, b, epi, bn, out, v, splits)
        if epi == 2:
            ck.add("E", out, P.exp_bias(acc, b), what, buf=buf)
        elif epi == 4:
            ck.add("E", out, P.exp_bias_relu(acc, b), what, buf=buf)
        else:
            e = P.gelu_in(acc, b)
            ck.add("gelu", out, P.gelu64(e), what, buf=buf, floor=P.gelu_floor(e))
    elif epi == 1:
        g, u = acc[:, : N // 2], acc[:, N // 2:]
        buf, out = P.out_buffer(M, N // 2, DEV)
        hip.gemm(x, w, None, 1, bn, out, v, splits)
        ck.add("swiglu", out, P.swiglu64(g, u), what, buf=buf, floor=P.swiglu_floor(u))
    elif epi == 6:
        r0 = P.int_matrix(M, N, -32, 32, M + K, DEV)
        buf, r = P.out_buffer(M, N, DEV)
        r.copy_(r0)
        ss = torch.full((N // 256, M + 5), float("nan"), device=DEV)
        hip.gemm_fused(x, w, 6, bn, None, v, splits, resid=r, ss_out=ss)
        new, ss_want = P.exp_resid(acc, r0)
        ck.add("E", r, new, what + ": residual", buf=buf)
        ck.add("E", ss[:, :M], ss_want.float(), what + ": sums of squares")
        ck.add("E", torch.isnan(ss[:, M:]), torch.ones(N // 256, 5, dtype=torch.bool, device=DEV), what + ": ss columns past M")
    else:  # 7: QKV at hd 128, interleaved pairs, k rotated in the row as well
        Hq, Hkv, D, BS = N // 128 - 2, 1, 128, 16
        cs = P.rope_table(64, D, DEV)
        pos = (torch.arange(M, device=DEV) % 3 == 1).int() * 37
        slots = torch.arange(M, dtype=torch.int32, device=DEV) * 2 + 1
        slots[M // 2] = -1
        kc = torch.full(((2 * M + 1) // BS + 2, Hkv, BS, D), P.SENTINEL, dtype=BF, device=DEV)
        vc = kc.clone()
        buf, out = P.out_buffer(M, N, DEV)
        hip.gemm_fused(x, w, 7, bn, out, v, splits, positions=pos, cos_sin=cs, slots=slots, k_cache=kc, v_cache=vc, hq=Hq,
                       hkv=Hkv, hd=D)
        ck.add("E", ((buf != P.SENTINEL).sum() - (out != P.SENTINEL).sum()).view(1, 1),
               torch.zeros(1, 1, dtype=torch.long, device=DEV), what + ": elements written outside the result")
        _qkv_checks(ck, what, out, kc, vc, acc, pos, slots, cs, Hq, Hkv, D, False, True)


@pytest.mark.parametrize("M", PREFILL_M)
def test_prefill_epilogues(hip, M):
    """Every epilogue on an exact small accumulator: bias, bias + ReLU and RESID bit-exact, GELU and
    SwiGLU to their measured tolerance, elementwise; QKV at head size 128."""
    ck = Checks()
    for epi in (2, 3, 4, 1, 6, 7):
        N = 512 if epi == 1 else PREFILL_N
        ran = 0
        for kt in (1, 2, 3, 4, 9):
            K = 64 * kt
            x, w, acc = _low(M, N, K, seed=epi)
            for v, bn in _cfgs(hip, M, N, K, epi):
                _epilogue_case(hip, ck, M, N, K, epi, v, bn, 1, x, w, acc)
                ran += 1
        assert ran >= 20, f"epilogue {epi}: only {ran} configurations ran"
        ck.finish()


@pytest.mark.parametrize("M", PREFILL_M)
@pytest.mark.parametrize("ks", [2, 3, 4, 8])
def test_prefill_splitk(hip, M, ks):
    """Split-K with even and uneven K ranges: D, R with its terms in the first and the last split
    (the first split's partial itself unrepresentable in bf16), the bias epilogues and RESID in the
    reduce kernels."""
    N = PREFILL_N
    ck = Checks()
    for kt in (2 * ks, 2 * ks + 1, 3 * ks, 3 * ks + 1):
        K = 64 * kt
        x, w, acc = _dense(M, N, K, 1.0)
        pairs = [(5, K - 4), (5, K - 4, 64 + 40)]  # K-tiles 0 and 1: the first split; the last K-tile: the last
        rs = []
        for start in range(0, len(pairs), M):
            xr, wr = P.rounding(M, N, K, pairs, start, DEV)
            rs.append((xr, wr, P.rbf(P.expect(xr, wr))))
        xl, wl, accl = _low(M, N, K, seed=ks)
        cfgs = [c for c in PREFILL_CFGS if hip.gemm_supported(M, N, K, 0, c[1], ks, c[0])]
        want_cfgs = 6 + (3 if kt >= 3 * ks else 0)
        assert len(cfgs) >= want_cfgs, f"split {ks} at {kt} K-tiles: {cfgs}"
        for v, bn in cfgs:
            buf, out = P.out_buffer(M, N, DEV)
            hip.gemm(x, w, None, 0, bn, out, v, ks)
            ck.add("D", out, P.rbf(acc), f"gemm split {ks} D M{M} K{K} variant {v} bn {bn}", buf=buf)
            for xr, wr, want in rs:
                buf, out = P.out_buffer(M, N, DEV)
                hip.gemm(xr, wr, None, 0, bn, out, v, ks)
                ck.add("R", out, want, f"gemm split {ks} R M{M} K{K} variant {v} bn {bn}", buf=buf)
            for epi in (2, 3, 4, 6):
                if hip.gemm_supported(M, N, K, epi, bn, ks, v):
                    _epilogue_case(hip, ck, M, N, K, epi, v, bn, ks, xl, wl, accl)
                else:
                    assert epi == 6 and bn == 192, f"epi {epi} split {ks} variant {v} bn {bn} rejected"
        ck.finish()


@pytest.mark.parametrize("kt", [3, 4, 5, 16, 17])
def test_prefill_persistent_walk(hip, kt):
    """gemm1w's persistent walk (on at 3 to 16 K-tiles, off at 17) over 43 / 58 / 87 row tiles x 12
    column tiles with an M tail: every tile of D."""
    M, N, K = 11009, 3072, 64 * kt
    x, w, acc = _dense(M, N, K, 1.0)
    want = P.rbf(acc)
    for v in (3, 4, 5):
        assert hip.gemm_supported(M, N, K, 0, 256, 1, v)
        buf, out = P.out_buffer(M, N, DEV)
        hip.gemm(x, w, None, 0, 256, out, v)
        ck = Checks()
        ck.add("D", out, want, f"persistent walk kt {kt} variant {v}", buf=buf)
        ck.finish()


@pytest.mark.parametrize("variant", [6, 7])
def test_prefill_column_split(hip, variant):
    M, N, K = 4096, 6144, 192
    assert ops._split_applies(M, N, 0), "the shape must engage the column split"
    assert hip.gemm_supported(M, N, K, 0, 256, 1, variant)
    x, w, acc = _dense(M, N, K, 1.0)
    buf, out = P.out_buffer(M, N, DEV)
    hip.gemm(x, w, None, 0, 256, out, variant)
    ck = Checks()
    ck.add("D", out, P.rbf(acc), f"column split variant {variant}", buf=buf)
    xh, wh, k0, side = P.one_hot(M, N, K, 0, DEV)
    buf, out = P.out_buffer(M, N, DEV)
    hip.gemm(xh, wh, None, 0, 256, out, variant)
    ck.add("H", out, P.rbf(P.one_hot_expect(xh, wh, k0, side)), f"column split H variant {variant}", buf=buf, k0=k0, side=side)
    ck.finish()


@pytest.mark.parametrize("MNK", [(4352, 4096, 4096), (4300, 6144, 4096)])
def test_prefill_streamk(hip, MNK):
    """Stream-K partial tiles summed in f32: D at density 1 / 16 is bit-exact, equals the plain
    tiling, and no wait gave up."""
    M, N, K = MNK
    x, w, acc = _dense(M, N, K, 1.0 / 16)
    want = P.rbf(acc)
    engaged = 0
    try:
        for v, bn in PREFILL_CFGS[:9]:
            if not hip.gemm_supported(M, N, K, 0, bn, 1, v):
                continue
            hip.gemm_streamk(0)
            plain = hip.gemm(x, w, None, 0, bn, None, v)
            hip.gemm_streamk(1)
            n0 = hip.gemm_streamk(-2)
            buf, out = P.out_buffer(M, N, DEV)
            hip.gemm(x, w, None, 0, bn, out, v)
            engaged += hip.gemm_streamk(-2) > n0
            ck = Checks()
            ck.add("D", out, want, f"stream-K M{M} N{N} variant {v} bn {bn}", buf=buf)
            ck.add("D", plain, want, f"stream-K off M{M} N{N} variant {v} bn {bn}")
            ck.finish()
            assert torch.equal(out, plain)
            assert hip.gemm_streamk(-1) == 0, "a stream-K wait gave up"
        assert engaged, "no configuration engaged stream-K"
    finally:
        hip.gemm_streamk(1)


# ================================================================ routing
@pytest.mark.parametrize("NK", [(512, 1024), (512, 2048)])
def test_linear_routing_sweep(hip, NK):
    """ops.linear at every M from 1 to 300: bit-exact across every hand-off between the GEMV (K 2048;
    K 1024 has no GEMV plan), the weight-streaming kernel and the prefill GEMM, static routing."""
    N, K = NK
    x, w, acc = _dense(300, N, K, 1.0)
    want = P.rbf(acc)
    saved = dict(ops._DECODE_TABLE)
    ops._DECODE_TABLE.clear()
    kinds = set()
    ck = Checks()
    try:
        for M in range(1, 301):
            xm = x[:M]
            kinds.add("gemv" if ops._gemv_ok(xm, w, 0) else ops._decode_gemm_kind(xm, w, False))
            ck.add("D", ops.linear(xm, w), want[:M], f"ops.linear M{M} N{N} K{K}")
        ck.finish()
    finally:
        ops._DECODE_TABLE.clear()
        ops._DECODE_TABLE.update(saved)
    assert {"ws", None} <= kinds and (("gemv" in kinds) == (K == 2048)), kinds
