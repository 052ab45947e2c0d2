"""Structured GEMM inputs whose float64 answer pins every single product, the rounding of the store
and the arithmetic of each epilogue.

randn activations against randn * 0.05 weights at K >= 4096 need a tolerance of many products: a
kernel that drops, doubles or mispairs one product (or a whole 8-element chunk) for one tile, one
K-step or one split boundary stays far below it.  Small integers and halves are exact in bf16, their
products are exact in f32, and their sums are exact in f32 in any order while |sum| < 2^24 -- so with
the inputs below the accumulator of every kernel (MFMA 16x16x32, the GEMV's fmaf on widened bf16,
split-K f32 slabs, stream-K partial tiles, LDS cross-wave sums, wave_sum) must EQUAL the integer
answer, and the only rounding left is the documented one of the store:

D "dense sign"  x in {-1, +1}, w in {-1, 0, +1} (``density`` = share of non-zeros): every product that
                exists moves the sum by +-1.  An error of +-1 is certain to show only where
                |expected| <= 256 (bf16 holds every integer up to there): at most 5 % of the expected
                elements may lie outside (asserted).  For the epilogues K * density <= 256 and every
                |acc| <= 192 (asserted): the accumulator is an exact small integer.
H "one-hot K"   the operand with more rows has ONE +-1 / +-2 per row at k0(row) = (row + shift) % K,
                the other one the asymmetric pattern (37 row + 11 k) % 251 - 125: the expected element is
                the selected one times 1 or 2, so a failure names the k that was dropped, doubled or
                mispaired.
R "rounding"    x rows of two 1s at (k1, k2), w[n, k1] in +-{256, 258, ..., 510}, w[n, k2] in
                +-{0.5, 1, 1.5}: the sum is exact in f32, not representable in bf16 and includes exact
                ties -- the expected matrix differs from truncation, round-half-up and
                round-half-away (asserted).  k1 and k2 sit in different K-steps / splits, so the sum
                crosses the reduction.  Rows of three 1s (k3 beside k1, w[n, k3] = +-1) make the
                first split's partial itself unrepresentable: rounding a partial before the sum shows.

Epilogues on an exact accumulator: none / bias / bias + ReLU / RESID / GEMV mode 1 are bit-exact; SwiGLU,
GELU, RoPE and the RMSNorm tail are compared elementwise against the float64 answer in bf16 ulps of
that answer (never of the matrix maximum), see ULPS below.

Plain torch; the GPU tests import this module as a sibling and pass ``device``.
"""
import math

import torch

BF = torch.bfloat16
SENTINEL = -24576.0  # fills the output buffers around the result (exact in bf16, no kernel output)
ACC_CAP = 192  # |accumulator| of the epilogue probes
SENS_CAP = 256  # bf16 holds every integer up to here
ERF_ABS = 1.5e-7  # csrc/common.h lk_fast_erf: Abramowitz & Stegun 7.1.26

# --- tolerances -------------------------------------------------------------------------------
# |got - want| <= ULPS[kind] * ulp(want) + floor, elementwise; ulp() = the bf16 spacing at the float64
# answer.  ULPS = twice the worst error of the CPU emulations below (the documented f32 arithmetic
# of the kernels, rounded where they round) against the float64 answer, over the whole domain the
# GPU tests can reach -- every integer accumulator pair in [-ACC_CAP, ACC_CAP]^2 (SwiGLU), every
# integer bias sum in [-256, 256] (GELU), every such pair against every (cos, sin) of ROPE_POS at
# D 64 and 128 (RoPE), every row of norm_cases() over NORM_CASES (RMSNorm tail) -- rounded up in the third digit.
# The factor 2 is for __expf / v_rcp / v_rsq and FMA contraction, which the emulations do not
# model.  Measured by measure_ulps() (tests/test_gemm_probes_cpu.py asserts these are 2 x what it
# measures): SwiGLU 1.267 (two roundings: silu to bf16, then the product), GELU 0.463, RoPE 0.5 (one
# rounding of an f32 value whose own error is in the floor), RMSNorm tail 1.373 (x * inv rounded to
# bf16, then the product).
MEASURED = {"swiglu": 1.267, "gelu": 0.463, "rope": 0.5, "norm": 1.373}
ULPS = {k: 2 * v for k, v in MEASURED.items()}
# floors, where the result can cancel or sit near zero:
#   GELU  0.5 e (1 + erf): the erf's absolute error times |e| / 2
#   RoPE  x1 c - x2 s in f32: 4 * 2^-24 * (|x1 c| + |x2 s|)
#   SwiGLU silu(g) = g / (1 + exp(-g)): exp(-g) overflows f32 past -g = 88.72, where the kernel's silu is 0
#         and the true one at most 88.72 / FLT_MAX < 2^-121: that times |u|
SILU_TINY = 2.0 ** -121
ROPE_POS = (0, 37)
ROPE_THETA = 500000.0
# (M, S, BN): the fused RMSNorm tail of the weight-streaming GEMM, N = NORM_N, K = 64 * S * 3
NORM_N = 384
NORM_CASES = [(M, S, BN) for M in (1, 2, 4) for S in (2, 4, 8) for BN in (64, 128)]
NORM_EPS = 1e-5


def ulp(x):
    """Spacing of bf16 at |x| (float64 tensor): 2^(floor(log2 |x|) - 7); 0 at 0."""
    _, e = torch.frexp(x.abs())
    # the power of two from its exponent bits: torch.ldexp is not exact on every device (2^-9 came out
    # one float64 ulp short on the GPU, which turned exact ties of round_bf16 into near-ties)
    p = ((e.long() + (1023 - 8)).clamp(1, 2046) << 52).view(torch.float64)
    return torch.where(x == 0, torch.zeros_like(x), p)


def round_bf16(e, mode="rne"):
    """float64 -> the bf16 grid (as float64): rne, trunc (toward zero), half_up (ties toward +inf),
    half_away (ties away from zero)."""
    e = e.double()
    u = ulp(e)
    q = torch.where(u > 0, e / u.clamp_min(1e-300), torch.zeros_like(e))
    if mode == "rne":
        q = torch.round(q)
    elif mode == "trunc":
        q = torch.trunc(q)
    elif mode == "half_up":
        q = torch.floor(q + 0.5)
    elif mode == "half_away":
        q = torch.sign(q) * torch.floor(q.abs() + 0.5)
    else:
        raise ValueError(mode)
    return q * u


def rbf(e):
    """One round-to-nearest-even to bf16 of an f32-exact float64 value (the kernels' store)."""
    f = e.float()
    assert torch.equal(f.double(), e.double()), "the value is not exact in f32"
    return f.to(BF)


def _exact(t, what):
    assert torch.equal(t.to(BF).double(), t.double()), f"{what} does not survive a bf16 round trip"
    return t.to(BF)


def expect(x, w):
    """float64 x w^T on the inputs' device."""
    return x.double() @ w.double().t()


# --- builders ---------------------------------------------------------------------------------
def dense_sign(M, N, K, density=1.0, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * K + N)
    x = torch.randint(0, 2, (M, K), generator=g, dtype=torch.int8) * 2 - 1
    w = torch.randint(0, 2, (N, K), generator=g, dtype=torch.int8) * 2 - 1
    if density < 1.0:
        w = w * (torch.rand(N, K, generator=g) < density).to(torch.int8)
    assert bool((x != 0).all())
    return _exact(x.to(device).float(), "x"), _exact(w.to(device).float(), "w")


def epi_density(K):
    return min(1.0, SENS_CAP / K)


def assert_sensitive(e, cap=0.05):
    share = float((e.abs() > SENS_CAP).double().mean())
    assert share <= cap, f"{share:.3%} of the expected elements lie outside [-256, 256]"
    return share


def assert_acc_cap(e):
    m = float(e.abs().max()) if e.numel() else 0.0
    assert m <= ACC_CAP, f"max |acc| = {m} > {ACC_CAP}"


def pattern(rows, K, device="cpu"):
    r = torch.arange(rows, device=device)[:, None]
    k = torch.arange(K, device=device)[None, :]
    return _exact(((37 * r + 11 * k) % 251 - 125).float(), "pattern")


HOT_VALS = (1.0, -1.0, 2.0, -2.0)


def one_hot(M, N, K, shift=0, device="cpu"):
    """-> x, w, k0, side.  side 'w': w[n, k0[n]] = +-1 / +-2 (N >= M); 'x': x[m, k0[m]] (M > N).
    k0(row) = (row + shift) % K walks every k once rows >= K (else: several launches, shifted)."""
    side = "w" if N >= M else "x"
    rows, other = (N, M) if side == "w" else (M, N)
    idx = torch.arange(rows, device=device)
    k0 = (idx + shift) % K
    val = torch.tensor(HOT_VALS, device=device)[(3 * idx + idx // 7) % 4]
    hot = torch.zeros(rows, K, device=device)
    hot[idx, k0] = val
    hot, pat = _exact(hot, "one-hot"), pattern(other, K, device)
    return (pat, hot, k0, side) if side == "w" else (hot, pat, k0, side)


def one_hot_expect(x, w, k0, side):
    """The selected element times the one-hot value, without a matmul (float64)."""
    if side == "w":
        n = torch.arange(w.shape[0], device=w.device)
        return x.double()[:, k0] * w.double()[n, k0][None, :]
    m = torch.arange(x.shape[0], device=x.device)
    return x.double()[m, k0][:, None] * w.double()[:, k0].t()


def hot_shifts(rows, K):
    """Shifts after which k0 has walked all of K."""
    return list(range(0, K, rows)) if rows < K else [0]


def split_pairs(K, S=1):
    """(k1, k2) pairs and (k1, k2, k3) triples for R over S equal K-splits: k1 in the first K-step of
    split i, k3 in its last one, k2 in the last K-step of split (i + 1) % S (S = 1: k1 in the first
    K-step, k2 and k3 in the last).  Offsets inside a 64-element K-step: k1 5.., k3 40.., k2 53..60."""
    ks = K // S
    assert ks >= 64 and ks * S == K
    out = []
    for i in range(S):
        j, o = (i + 1) % S, i % 8
        k1, k3, k2 = i * ks + 5 + o, i * ks + ks - 24 + o, j * ks + ks - 4 - o
        out += [(k1, k2), (k1, k2, k3)]
    return out


SMALLS = (0.5, -0.5, 1.0, -1.0, 1.5, -1.5)


def rounding(M, N, K, pairs, start=0, device="cpu"):
    """Row m of x has 1s at pairs[(m + start) % len(pairs)]; see the header."""
    x = torch.zeros(M, K, device=device)
    w = torch.zeros(N, K, device=device)
    k1s, k2s, k3s = {p[0] for p in pairs}, {p[1] for p in pairs}, {p[2] for p in pairs if len(p) == 3}
    assert not (k1s & k2s) and not (k3s & (k1s | k2s)), "a column holds one kind of value"
    g = torch.Generator().manual_seed(7919 * K + N)  # (seeded: the same columns for every M and start)
    sm = torch.tensor(SMALLS)
    for k1 in sorted(k1s):
        sign = 1.0 - 2.0 * torch.randint(0, 2, (N,), generator=g)
        w[:, k1] = (sign * (256 + 2 * torch.randint(0, 128, (N,), generator=g))).to(device)
    for k2 in sorted(k2s):
        w[:, k2] = sm[torch.randint(0, 6, (N,), generator=g)].to(device)
    for k3 in sorted(k3s):
        w[:, k3] = (1.0 - 2.0 * torch.randint(0, 2, (N,), generator=g)).to(device)
    rows = [m for m in range(M) for _ in pairs[(m + start) % len(pairs)]]
    cols = [k for m in range(M) for k in pairs[(m + start) % len(pairs)]]
    x[torch.tensor(rows, device=device), torch.tensor(cols, device=device)] = 1.0
    return _exact(x, "x"), _exact(w, "w")


def assert_rounding_separates(e):
    """The RNE answer differs from truncation, round-half-up and round-half-away."""
    want = round_bf16(e, "rne")
    for mode in ("trunc", "half_up", "half_away"):
        assert bool((round_bf16(e, mode) != want).any()), f"R does not tell RNE from {mode}"
    assert bool((want != e).any())


# --- output buffers ---------------------------------------------------------------------------
def out_buffer(M, N, device="cpu", pad_rows=3, pad_cols=8, offset=0):
    """-> (buf, view): a SENTINEL-filled [M + pad_rows, N + pad_cols] buffer (flat, plus
    ``offset`` elements in front) and the [M, N] view the kernel writes (ldo = N + pad_cols)."""
    ld = N + pad_cols
    buf = torch.full((offset + (M + pad_rows) * ld + 8,), SENTINEL, dtype=BF, device=device)
    return buf, buf.as_strided((M, N), (ld, 1), offset)


def check_sentinel(buf, view, what=""):
    """Everything of buf outside view still holds SENTINEL."""
    M, N = view.shape
    ld = view.stride(0)
    off = view.storage_offset() - buf.storage_offset()
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    keep.as_strided((M, N), (ld, 1), off).fill_(False)
    bad = keep & (buf != SENTINEL)
    if bool(bad.any()):
        i = int(bad.nonzero()[0]) - off
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the result were written, the first at "
                             f"row {i // ld}, column {i % ld} of a [{M}, {N}] result")


# --- epilogue expectations from an exact accumulator (float64 in, float64 / bf16 out) -------------
def exp_none(acc):
    return rbf(acc)


def exp_bias(acc, b):
    return rbf(acc + b.double()[None, :])


def exp_bias_relu(acc, b):
    return torch.relu(exp_bias(acc, b).float()).to(BF)


def exp_resid(acc, r):
    """-> (new r bf16, ss f64 [N / 256, M]): r = bf16(r + bf16(acc)), per-256-column sums of squares."""
    new = rbf(rbf(acc).double() + r.double())
    M, N = new.shape
    ss = new.double().pow(2).view(M, N // 256, 256).sum(-1).t().contiguous() if N % 256 == 0 else None
    return new, ss


def gelu_in(acc, b):
    return exp_bias(acc, b).double()


def gelu64(e):
    return 0.5 * e * (1.0 + torch.erf(e / math.sqrt(2.0)))


def gelu_floor(e):
    return ERF_ABS * e.abs() / 2


def silu64(g):
    return g / (1.0 + torch.exp(-g))


def swiglu64(g, u):
    return silu64(rbf(g).double()) * rbf(u).double()


def swiglu_floor(u):
    return SILU_TINY * rbf(u).double().abs()


def rotate64(x1, x2, c, s):
    """-> (y1, y2, floor1, floor2) of the rotation of (x1, x2) by (c, s), float64."""
    x1, x2, c, s = x1.double(), x2.double(), c.double(), s.double()
    f = 4 * 2.0 ** -24
    return x1 * c - x2 * s, x2 * c + x1 * s, f * ((x1 * c).abs() + (x2 * s).abs()), f * ((x2 * c).abs() + (x1 * s).abs())


def rope_table(max_pos, D, device="cpu"):
    """[max_pos, D] f32 = [cos | sin] over D / 2 frequencies (ops.rope_cos_sin's table)."""
    inv = 1.0 / (ROPE_THETA ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    f = torch.outer(torch.arange(max_pos, dtype=torch.float64), inv)
    return torch.cat([f.cos(), f.sin()], dim=-1).float().to(device)


def rope_expect(qkv, pos, cs, Hq, Hkv, D, neox, rotate_k):
    """qkv: f64 [M, (Hq + 2 Hkv) D] of bf16-exact values.  -> (want, floor) f64 with the Hq (and,
    rotate_k, the Hkv key) heads rotated by cs[pos]; interleaved pairs unless neox."""
    M = qkv.shape[0]
    nrot = Hq + (Hkv if rotate_k else 0)
    want, floor = qkv.clone(), torch.zeros_like(qkv)
    h = qkv[:, : nrot * D].reshape(M, nrot, D)
    c = cs[pos.long()][:, None, : D // 2].double()
    s = cs[pos.long()][:, None, D // 2:].double()
    x1, x2 = (h[..., : D // 2], h[..., D // 2:]) if neox else (h[..., 0::2], h[..., 1::2])
    y1, y2, f1, f2 = rotate64(x1, x2, c, s)
    if neox:
        y, f = torch.cat([y1, y2], -1), torch.cat([f1, f2], -1)
    else:
        y, f = torch.stack([y1, y2], -1).flatten(-2), torch.stack([f1, f2], -1).flatten(-2)
    want[:, : nrot * D] = y.reshape(M, nrot * D)
    floor[:, : nrot * D] = f.reshape(M, nrot * D)
    return want, floor


def norm64(v, g, eps=NORM_EPS):
    v = v.double()
    return v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps) * g.double()[None, :]


def norm_gamma(N, device="cpu"):
    return _exact(0.5 + (torch.arange(N, device=device) * 29 % 64).float() / 64, "gamma")


def int_vector(N, lo, hi, seed, device="cpu"):
    """Seeded integers in [lo, hi] as bf16 (a bias, one row of a residual)."""
    g = torch.Generator().manual_seed(seed)
    return _exact(torch.randint(lo, hi + 1, (N,), generator=g).float().to(device), "integers")


def int_matrix(M, N, lo, hi, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return _exact(torch.randint(lo, hi + 1, (M, N), generator=g).float().to(device), "integers")


def norm_cases(M, S, device="cpu"):
    """Inputs of one NORM_CASES entry, as (name, x, w, residual, gamma): D at low density, and H
    shifted until every k was selected."""
    K = 64 * S * 3
    res, gam = int_matrix(M, NORM_N, -32, 32, 11 * S + M, device), norm_gamma(NORM_N, device)
    x, w = dense_sign(M, NORM_N, K, epi_density(K), seed=S, device=device)
    out = [("D", x, w, res, gam)]
    for shift in hot_shifts(NORM_N, K):
        x, w, _, _ = one_hot(M, NORM_N, K, shift, device)
        out.append((f"H shift {shift}", x, w, res, gam))
    return out


# --- CPU emulations of the kernels' f32 arithmetic -----------------------------------------------
def _r(f):
    return f.to(BF).float()


def emu_swiglu(g, u):
    g = _r(g.float())
    return _r(g / (1.0 + torch.exp(-g))) * _r(u.float())


def emu_gelu(e):
    x = e.float()
    z = x * 0.70710678118654752
    a = z.abs()
    t = 1.0 / (0.3275911 * a + 1.0)
    p = 1.061405429 * t - 1.453152027
    p = p * t + 1.421413741
    p = p * t - 0.284496736
    p = p * t + 0.254829592
    y = 1.0 - p * t * torch.exp(-a * a)
    return 0.5 * x * (1.0 + torch.copysign(y, z))


def emu_rotate(x1, x2, c, s):
    x1, x2, c, s = x1.float(), x2.float(), c.float(), s.float()
    return x1 * c - x2 * s, x2 * c + x1 * s


def emu_norm(v, g, eps=NORM_EPS):
    v = v.float()
    inv = torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps)
    return _r(v * inv) * g.float()[None, :]


def excess_ulps(got, want, floor=None):
    """(|got - want| - floor) / ulp(want), elementwise, >= 0; inf where an expected zero (and a
    zero floor) is not an exact zero."""
    want = want.double()
    d = (got.double() - want).abs()
    if floor is not None:
        d = (d - floor.double()).clamp_min(0)
    u = ulp(want)
    inf = torch.full_like(d, float("inf"))
    return torch.where(u > 0, d / u.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), inf))


def measure_ulps():
    """Worst error of each emulation, rounded to bf16 as the kernels store it, in bf16 ulps of the
    float64 answer, over the domains named at ULPS."""
    out = {}
    r = torch.arange(-ACC_CAP, ACC_CAP + 1, dtype=torch.float64)
    g, u = r[:, None].expand(-1, r.numel()), r[None, :].expand(r.numel(), -1)
    out["swiglu"] = float(excess_ulps(emu_swiglu(g, u).to(BF), swiglu64(g, u), swiglu_floor(u)).max())
    e = torch.arange(-SENS_CAP, SENS_CAP + 1, dtype=torch.float64)
    out["gelu"] = float(excess_ulps(emu_gelu(e).to(BF), gelu64(e), gelu_floor(e)).max())
    worst = 0.0
    for D in (64, 128):
        cs = rope_table(max(ROPE_POS) + 1, D)
        for pos in ROPE_POS:
            c, s = cs[pos, : D // 2], cs[pos, D // 2:]
            x1, x2 = g[:, :, None], u[:, :, None]
            y1, y2, f1, f2 = rotate64(x1, x2, c, s)
            e1, e2 = emu_rotate(x1, x2, c, s)
            worst = max(worst, float(excess_ulps(e1.to(BF), y1, f1).max()), float(excess_ulps(e2.to(BF), y2, f2).max()))
    out["rope"] = worst
    worst = 0.0
    for M, S, _ in NORM_CASES:
        for _, x, w, res, gam in norm_cases(M, S):
            v, _ = exp_resid(expect(x, w), res)
            worst = max(worst, float(excess_ulps(emu_norm(v, gam).to(BF), norm64(v, gam)).max()))
    out["norm"] = worst
    return out


# --- checks -----------------------------------------------------------------------------------
def check(kind, got, want, what="", floor=None, k0=None, side=None):
    """kind D / H / R / E (an exact epilogue): got must equal want (bf16) bit for bit; swiglu / gelu /
    rope / norm: |got - want| <= ULPS[kind] * ulp(want) + floor with want in float64.  k0 / side
    (H): the failure names the k of the first wrong element."""
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite output"
    if kind in ULPS:
        x = excess_ulps(got, want, floor)
        bad = x > ULPS[kind]
    else:
        assert want.dtype == got.dtype, "exact probes compare like with like"
        bad = got != want
    if not bool(bad.any()):
        return
    idx = tuple(int(v) for v in bad.nonzero()[0])
    msg = (f"{what}: probe {kind}: {int(bad.sum())} of {bad.numel()} elements off; the first at {idx} "
           f"(16 x 16 tile {tuple(i // 16 for i in idx)}): got {float(got[idx])!r}, want {float(want[idx])!r}")
    if kind in ULPS:
        msg += f" ({float(x[idx]):.3g} ulps, {ULPS[kind]} allowed)"
    if k0 is not None:
        msg += f"; its k = {int(k0[idx[1] if side == 'w' else idx[0]])}"
    rows = bad.any(dim=1).nonzero().flatten().tolist()
    cols = bad.any(dim=0).nonzero().flatten().tolist()
    msg += f"; rows {rows[0]}..{rows[-1]} ({len(rows)}), columns {cols[0]}..{cols[-1]} ({len(cols)})"
    raise AssertionError(msg)
