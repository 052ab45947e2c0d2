"""Structured inputs for the row-wise kernels (csrc/norm.hip, rope_kv.hip, activation.hip, pooling.hip
and the vocab-parallel argmax key of sampling.hip) whose float64 answer pins every element.

The answer is computed in float64 and is built for the WHOLE buffer the kernel writes into:
wherever the kernel must not write, the answer holds SENTINEL (row padding beyond H, cache rows of
no slot, the V and unrotated-K columns of a qkv row keep their inputs).  It is rounded to bf16 where
a kernel rounds a value that f32 holds exactly -- the residual sum and x + bias -- so that ties pin
the rounding mode.  The kernels' other documented roundings (x * inv before the RMSNorm weight,
silu(g) before the product, the final store) round values that carry an f32 error: a rounded answer
would be a coin toss beside every tie, so there the answer stays the float64 value and the
roundings are part of the measured error of the emulation (as gemm_probes.py does for its
SwiGLU and RMSNorm tails).

Where the arithmetic is exact (spike rows' zeros, constant LayerNorm rows, the residual stream,
RoPE on the synthetic table, the KV caches, ReLU, CLS pooling without normalisation, row norms of
perfect squares) the comparison is bitwise.  Elsewhere

    |got - want| <= ULPS[kind] * ulp(want) + floor      elementwise,

with the ulp taken at the answer (bf16 spacing for bf16 outputs, f32 spacing for f32 outputs),
NaN answers met by NaN, infinite answers met exactly.

Plain torch; the GPU tests import this module as a sibling and pass ``device``.
tests/test_row_probes_cpu.py shows what these comparisons reject."""
import math

import torch

import gemm_probes as G
from gemm_probes import BF, ERF_ABS, SENTINEL, SILU_TINY, excess_ulps, round_bf16, ulp  # noqa: F401

# --- tolerances -------------------------------------------------------------------------------
# ULPS = twice the worst error of the f32 CPU emulations below (the kernels' documented arithmetic,
# rounded where they round) against the float64 answer over the whole domain the GPU tests reach;
# the factor 2 is for __expf / v_rcp / v_rsq and FMA contraction, which the emulations do not model
# (the reason and the margin of gemm_probes.py).  Measured by measure_ulps(), rounded up in the
# third digit; tests/test_row_probes_cpu.py asserts that the constants equal what it measures.
#   rms      every row of norm_rows(H) and resid_rows(H), H in NORM_H, eps NORM_EPS
#   ln       every row of ln_rows(H) with and without bias, resid_rows(H), embed_tables(H), H in NORM_H
#   silu     every bf16 bit pattern as the gate against every value of UPS
#   gelu, gelu_tanh   every bf16 bit pattern, without a bias and plus every value of ACT_BIAS
#   rope     |x| <= 32 integers against ref.rope_cos_sin(theta 500000) at ROPE_POS, every D of ROPE_D
#   pool     (f32 ulps) pool_hidden(H) over POOL_LENS, H in POOL_H, both modes, normalize on and off
# Measured: rms 1.375 (x * inv rounded to bf16, then the product rounded), ln 0.554 and gelu 0.5 (one
# rounding of an f32 value whose own error is in the floor), silu 1.248 (two roundings), rope 0.5,
# pool 1.638 f32 ulps (the division, the root, the reciprocal and the product).
MEASURED = {"rms": 1.375, "ln": 0.554, "silu": 1.248, "gelu": 0.5, "gelu_tanh": 0.5, "rope": 0.5, "pool": 1.638}
ULPS = {k: 2 * v for k, v in MEASURED.items()}
F32_KINDS = ("pool", "rownorm")
ULPS_FIXED = {"rownorm": 1.0}  # set by the probe: the root of a perfect square, within 1 f32 ulp
# floors, derived (not measured), where the answer cancels or sits near zero:
#   rope       4 * 2^-24 * (|x1 c| + |x2 s|): the f32 products before they cancel (gemm_probes.rotate64)
#   gelu       0.5 |e| ERF_ABS: the absolute error of 1 + erf (A&S 7.1.26; for the tanh form the f32
#              rounding of 1 + tanh, <= 2^-24, is below it) times |e| / 2
#   silu       SILU_TINY |u|: exp(-g) overflows f32 past -g = 88.72 where the kernel's silu is 0;
#              2^-126 |u| for subnormal gates (silu(g) ~ g / 2 may be flushed to zero)
#   ln         4 * 2^-24 * (|(v - mean) inv g| + |b|): the f32 product and its cancellation against the bias
LN_FLOOR = 4 * 2.0 ** -24
SUBNORMAL = 2.0 ** -126
BF_TINY = 2.0 ** -133  # spacing of the bf16 subnormals
NORM_EPS = 1e-5
NORM_H = (8, 512, 520, 1016, 1024, 1032, 1536, 2040, 2048, 4096, 4104, 8192, 8200, 16384)
ROPE_D = (16, 32, 64, 96, 128, 256)
ROPE_THETA = 500000.0
ROPE_MAX_POS = 64
ROPE_POS = (0, 1, 37, ROPE_MAX_POS - 1)
POOL_H = (8, 768, 1024, 1032, 2048, 2056, 4096)
POOL_LENS = (3, 0, 1, 40, 0, 2)  # the last sequence is all zeros
UPS = (1.0, -2.0, 0.5, 3.0)
ACT_BIAS = (0.5, -1.5, 1.0, 256.0, -0.25, 3.0, -0.125, 128.0)


def ulp_bf(x):
    """bf16 spacing at |x| (float64), the subnormal spacing below 2^-126, 0 at 0."""
    u = ulp(x)
    return torch.where(x == 0, u, u.clamp_min(BF_TINY))


def ulp_f32(x):
    u = ulp(x) * 2.0 ** -16
    return torch.where(x == 0, u, u.clamp_min(2.0 ** -149))


def to_bf16(e):
    """float64 -> the nearest bf16 value (as float64), ties to even; subnormals, overflow to inf
    and NaN included (gemm_probes.round_bf16 covers the normal range only)."""
    e = e.double()
    fin = torch.isfinite(e)
    z = torch.where(fin, e, torch.zeros_like(e))
    u = ulp(z).clamp_min(BF_TINY)
    q = torch.round(z / u) * u
    q = torch.where(q.abs() >= 2.0 ** 128, torch.sign(q) * float("inf"), q)
    return torch.where(fin, q, e)


def final64(e):
    """The unrounded float64 answer of a bf16 store: +-inf where the store overflows."""
    e = e.double()
    return torch.where(e.abs() >= 2.0 ** 128 * (1 - 2.0 ** -9), torch.sign(e) * float("inf"), e)


def exact_bf16(e, what="the answer"):
    """float64 -> bf16 of a value bf16 holds exactly."""
    b = e.to(BF)
    assert torch.equal(b.double(), e.double()), f"{what} is not exact in bf16"
    return b


def excess(kind, got, want, floor=None):
    """(|got - want| - floor) / ulp(want) elementwise in the output's own ulps; inf where a NaN, an
    infinite or a SENTINEL answer is not met exactly."""
    want = want.double()
    g = got.double()
    u = ulp_f32(want) if kind in F32_KINDS else ulp_bf(want)
    d = (g - want).abs()
    if floor is not None:
        d = (d - floor.double()).clamp_min(0)
    inf = torch.full_like(d, float("inf"))
    zero = torch.zeros_like(d)
    x = torch.where(u > 0, d / u.clamp_min(1e-300), torch.where(d == 0, zero, inf))
    special = ~torch.isfinite(want) | (want == SENTINEL)
    same = torch.where(torch.isnan(want), torch.isnan(g), g == want)
    x = torch.where(special, torch.where(same, zero, inf), x)
    return torch.where(torch.isnan(x), inf, x)


def limit(kind):
    return ULPS_FIXED[kind] if kind in ULPS_FIXED else ULPS[kind]


def bad(kind, got, want, floor=None):
    """Boolean verdict per element: kind 'E' bitwise-equal values (+0 == -0), else the ulp rule."""
    assert got.shape == want.shape, f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    if kind == "E":
        return got.double() != want.double()
    return excess(kind, got, want, floor) > limit(kind)


def describe(kind, got, want, floor=None, what=""):
    b = bad(kind, got, want, floor)
    if not bool(b.any()):
        return f"{what}: ok"
    idx = tuple(int(v) for v in b.nonzero()[0])
    msg = f"{what}: {int(b.sum())} of {b.numel()} elements off; the first at {idx}: got {float(got[idx])!r}, want {float(want[idx])!r}"
    if kind != "E":
        msg += f" ({float(excess(kind, got, want, floor)[idx]):.4g} ulps, {limit(kind)} allowed)"
    return msg


def check(kind, got, want, what="", floor=None):
    if bool(bad(kind, got, want, floor).any()):
        raise AssertionError(describe(kind, got, want, floor, what))


def padded(rows, cols, device="cpu", dtype=BF, pad_cols=8, pad_rows=1):
    """-> (buf [rows + pad_rows, cols + pad_cols] of SENTINEL, its [rows, cols] view)."""
    buf = torch.full((rows + pad_rows, cols + pad_cols), SENTINEL, dtype=dtype, device=device)
    return buf, buf[:rows, :cols]


def in_padded(x, pad_cols=8):
    """x copied into a SENTINEL buffer with a row stride of cols + pad_cols -> (buf, view)."""
    buf, view = padded(x.shape[0], x.shape[1], x.device, x.dtype, pad_cols)
    view.copy_(x)
    return buf, view


def want_padded(want, buf):
    """The float64 answer for the whole buffer: ``want`` inside, SENTINEL around it."""
    full = torch.full(buf.shape, SENTINEL, dtype=torch.float64, device=buf.device)
    full[: want.shape[0], : want.shape[1]] = want
    return full


# =============================================================================== norms
def row_cfg(H):
    """(waves, vectors per thread) of csrc/rowcfg.h."""
    nvec = H // 8
    nw = 4 if nvec > 128 else (2 if nvec == 128 else 1)
    return nw, (nvec + nw * 64 - 1) // (nw * 64)


def spike_vectors(H):
    """Vector indices the spike walks: all of them up to H 2048; above 0, 1, both sides of every
    multiple of 64 * nw, the last two and a stride-17 sample."""
    nvec = H // 8
    if H <= 2048:
        return list(range(nvec))
    nw, _ = row_cfg(H)
    s = {0, 1, nvec - 2, nvec - 1} | set(range(0, nvec, 17))
    for m in range(64 * nw, nvec, 64 * nw):
        s |= {m - 1, m}
    return sorted(s)


def gamma(H, device="cpu"):
    c = torch.arange(H, device=device)
    return exact_bf16((((13 * c + c // 8) % 61) - 30).double() / 16, "gamma")


def beta(H, device="cpu"):
    c = torch.arange(H, device=device)
    return exact_bf16((((7 * c + c // 8) % 33) - 16).double() / 8, "beta")


def dense(R, H, device="cpu", lo=125, mod=251):
    r = torch.arange(R, device=device)[:, None]
    c = torch.arange(H, device=device)[None, :]
    return ((37 * r + 11 * c) % mod - lo).double()


def spikes(H, device="cpu"):
    """One row per spike vector: zeros and one 16 at element row % 8 of vector c -> (x f64, columns)."""
    vec = torch.tensor(spike_vectors(H), device=device)
    r = torch.arange(vec.numel(), device=device)
    col = vec * 8 + r % 8
    x = torch.zeros(vec.numel(), H, dtype=torch.float64, device=device)
    x[r, col] = 16.0
    return x, col


def norm_rows(H, device="cpu"):
    """RMSNorm inputs (bf16): the spike rows, 3 dense rows, an all-zero row and a row of magnitude
    2^-10 (eps dominates) -> (x, number of spike rows)."""
    sp, _ = spikes(H, device)
    c = torch.arange(H, device=device)
    tiny = (1.0 - 2.0 * ((c * 5 + c // 8) % 3 == 0).double())[None, :] * 2.0 ** -10
    x = torch.cat([sp, dense(3, H, device), torch.zeros(1, H, dtype=torch.float64, device=device), tiny])
    return exact_bf16(x, "x"), sp.shape[0]


def resid_rows(H, device="cpu", R=4):
    """(x, residual) whose sums hold exact bf16 ties: |x| in {256, 258, .., 510}, residual in
    +-{0.5, 1, 1.5}."""
    r = torch.arange(R, device=device)[:, None]
    c = torch.arange(H, device=device)[None, :]
    x = (256 + 2 * ((7 * r + 3 * c + c // 8) % 128)).double() * (1.0 - 2.0 * ((r + c) % 3 == 1).double())
    res = torch.tensor(G.SMALLS, dtype=torch.float64, device=device)[(r + 5 * c + c // 8) % 6]
    return exact_bf16(x, "x"), exact_bf16(res.expand(R, H).contiguous(), "residual")


def add64(x, res):
    """The residual stream: bf16(x + residual), float64."""
    return to_bf16(x.double() + res.double())


def rms64(v, w, eps=NORM_EPS):
    v = v.double()
    inv = torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps)
    return v * inv * w.double()[None, :]


def ln_rows(H, device="cpu"):
    """LayerNorm inputs (bf16): the spike rows, two constant rows (3 and -0.75: zero variance), a row
    of mean 256 with deviations +-2 on every element (257 is no bf16 value), a row of 256 with only
    two deviating elements (variance 8 / H: E[x^2] - mean^2 loses it in f32), 2 dense rows
    -> (x, row index of the first constant row)."""
    sp, _ = spikes(H, device)
    c = torch.arange(H, device=device)
    one = torch.ones(1, H, dtype=torch.float64, device=device)
    alt = 256 + 2 * (1.0 - 2.0 * (c % 2).double())[None, :]
    two = 256 * one.clone()
    two[0, (3 * H) // 8 + 1] = 258
    two[0, H - 3] = 254
    x = torch.cat([sp, 3 * one, -0.75 * one, alt, two, dense(2, H, device, 30, 61)])
    return exact_bf16(x, "x"), sp.shape[0]


def ln64(v, g, b=None, eps=NORM_EPS):
    """-> (want, floor), float64; rows of zero variance give the bias (or 0) exactly."""
    v = v.double()
    mean = v.mean(-1, keepdim=True)
    d = v - mean
    inv = torch.rsqrt(d.pow(2).mean(-1, keepdim=True) + eps)
    t = d * inv * g.double()[None, :]
    bb = torch.zeros_like(t) if b is None else b.double()[None, :].expand_as(t)
    return t + bb, LN_FLOOR * (t.abs() + bb.abs())


def embed_tables(H, device="cpu", V=16, P=8):
    """tok [V, H], pos [P, H], typ [2, H] of small integers; tok[V - 1] + pos[0] + typ[0] is the
    constant 2 (zero variance: the output is the bias)."""
    tok = dense(V, H, device, 16, 33)
    pos = dense(P, H, device, 8, 17).flip(1)
    typ = dense(2, H, device, 4, 9)
    typ[0] = -2.0
    pos[0] = 1.0
    tok[V - 1] = 3.0
    return exact_bf16(tok, "tok"), exact_bf16(pos, "pos"), exact_bf16(typ, "typ")


def embed_ids(V=16, P=8, device="cpu"):
    ids = torch.tensor([0, V - 1, 5, V - 1, 1, 0, 9], dtype=torch.int32, device=device)
    pos_ids = torch.tensor([0, 0, P - 1, 3, 2, P - 1, 1], dtype=torch.int32, device=device)
    type_ids = torch.tensor([0, 0, 1, 1, 0, 1, 1], dtype=torch.int32, device=device)
    return ids, pos_ids, type_ids


def embed_sum(ids, pos_ids, type_ids, tok, pos, typ):
    e = tok.double()[ids.long()]
    if pos is not None:
        e = e + pos.double()[pos_ids.long()]
    if typ is not None:
        e = e + typ.double()[type_ids.long() if type_ids is not None else torch.zeros_like(ids).long()]
    return e


# f32 emulations; ``mutant`` injects one fault, ``c`` is the vector it hits
def _ss_mutant(sq, H, mutant, c):
    ss = sq.sum(-1, keepdim=True)
    if mutant == "drop":
        ss = ss - sq[:, 8 * c:8 * c + 8].sum(-1, keepdim=True)
    if mutant == "twice":
        ss = ss + sq[:, 8 * c:8 * c + 8].sum(-1, keepdim=True)
    return ss


def _width(H, mutant):
    nw, maxv = row_cfg(H)
    return float(nw * 64 * maxv * 8) if mutant == "padded_width" else float(H)


def _shift_w(w, mutant):
    return torch.roll(w, 8) if mutant == "weight_shift" else w


def emu_rms(v, w, eps=NORM_EPS, mutant=None, c=0):
    v = v.float()
    H = v.shape[1]
    ms = _ss_mutant(v * v, H, mutant, c) / _width(H, mutant)
    if mutant == "no_eps":
        inv = torch.rsqrt(ms)
    elif mutant == "eps_outside":
        inv = 1.0 / (torch.sqrt(ms) + eps)
    else:
        inv = torch.rsqrt(ms + eps)
    return ((v * inv).to(BF).float() * _shift_w(w.float(), mutant)[None, :]).to(BF)


def emu_ln(v, g, b=None, eps=NORM_EPS, mutant=None, c=0):
    v = v.float()
    H = v.shape[1]
    n = _width(H, mutant)
    s = v.sum(-1, keepdim=True)
    if mutant in ("drop", "twice"):
        s = s + (-1.0 if mutant == "drop" else 1.0) * v[:, 8 * c:8 * c + 8].sum(-1, keepdim=True)
    mean = s / n
    d = v - mean
    if mutant == "var_e2":
        var = (v * v).sum(-1, keepdim=True) / n - mean * mean
    else:
        var = _ss_mutant(d * d, H, mutant, c) / n
    if mutant == "no_eps":
        inv = torch.rsqrt(var)
    elif mutant == "eps_outside":
        inv = 1.0 / (torch.sqrt(var) + eps)
    else:
        inv = torch.rsqrt(var + eps)
    y = d * inv * _shift_w(g.float(), mutant)[None, :]
    if b is not None:
        y = y + _shift_w(b.float(), mutant)[None, :]
    return y.to(BF)


# =============================================================================== RoPE + KV write
TABLE_VALS = (0.0, 0.5, -0.5, 1.0, -1.0)


def synth_table(max_pos, D, device="cpu"):
    """[max_pos, D] f32 = [cos | sin] with entries from {0, +-0.5, +-1} in an asymmetric pattern of
    (position, frequency): every rotation of small integers is exact in f32 and in bf16."""
    p = torch.arange(max_pos, device=device)[:, None]
    f = torch.arange(D // 2, device=device)[None, :]
    vals = torch.tensor(TABLE_VALS, device=device)
    return torch.cat([vals[(3 * p + 5 * f + p * f + 3) % 5], vals[(2 * p + 3 * f + f // 8 + 1) % 5]], dim=-1).float()


def real_table(D, device="cpu", max_pos=ROPE_MAX_POS):
    return G.rope_table(max_pos, D, device)  # ops.reference.rope_cos_sin at theta 500000 (asserted on the CPU)


def qkv_rows(T, Hq, Hkv, D, device="cpu", pad=8):
    """-> (buf, view [T, (Hq + 2 Hkv) D] with a row stride ``pad`` larger): integers |x| <= 32 in an
    asymmetric pattern of (token, head, element), SENTINEL in the padding."""
    W = (Hq + 2 * Hkv) * D
    t = torch.arange(T, device=device)[:, None, None]
    h = torch.arange(Hq + 2 * Hkv, device=device)[None, :, None]
    e = torch.arange(D, device=device)[None, None, :]
    x = ((7 * t + 13 * h + 3 * e + t * e + h * (e // 8)) % 65 - 32).double().reshape(T, W)
    return in_padded(exact_bf16(x, "qkv"), pad)


def slot_list(T, NB, BS):
    """T distinct slots as a list (a permutation, not ascending) holding the last slot of the last
    block and, from T 2 on, slot 0; -1 at token 2 (T >= 3)."""
    last = NB * BS - 1
    cand = [last, 0] + [(5 * i + 3) % last for i in range(1, 2 * T + 2)]
    out = []
    for s in cand:
        if s not in out:
            out.append(s)
    out = out[:T]
    if T == 1:
        out = [last]
    if T >= 3:
        out[2] = -1
    assert len(out) == T and len(set(out)) == T
    return out


def slot_index(slots, BS, device="cpu"):
    """-> (tokens with a slot, their blocks, their offsets) as index tensors, from the host list."""
    tok = [t for t, s in enumerate(slots) if s >= 0]
    mk = lambda v: torch.tensor(v, dtype=torch.long, device=device)  # noqa: E731
    return mk(tok), mk([slots[t] // BS for t in tok]), mk([slots[t] % BS for t in tok])


def rope_want(qkv0, qs_buf, pos, cs, Hq, Hkv, D, neox, write_k_inplace, NB=0, BS=1, slots=None):
    """The float64 answers of rope_kv_ for whole buffers -> dict(row, row_floor[, kc, kc_floor, vc]):
    ``qkv0`` the [T, W] input view (bf16), ``qs_buf`` its padded buffer, ``slots`` a host list."""
    W = (Hq + 2 * Hkv) * D
    x = qkv0[:, :W].double()
    row, rfl = G.rope_expect(x, pos, cs, Hq, Hkv, D, neox, bool(write_k_inplace))
    out = {"row": want_padded(row, qs_buf), "row_floor": torch.zeros(qs_buf.shape, dtype=torch.float64, device=x.device)}
    out["row_floor"][: x.shape[0], :W] = rfl
    if slots is not None:
        rot, cfl = G.rope_expect(x, pos, cs, Hq, Hkv, D, neox, True)
        T = x.shape[0]
        sel, blk, off = slot_index(slots, BS, x.device)
        k = rot[:, Hq * D:(Hq + Hkv) * D].reshape(T, Hkv, D)[sel]
        kf = cfl[:, Hq * D:(Hq + Hkv) * D].reshape(T, Hkv, D)[sel]
        v = x[:, (Hq + Hkv) * D:].reshape(T, Hkv, D)[sel]
        kc = torch.full((NB, Hkv, BS, D), SENTINEL, dtype=torch.float64, device=x.device)
        vc, fl = kc.clone(), torch.zeros_like(kc)
        kc[blk, :, off] = k
        fl[blk, :, off] = kf
        vc[blk, :, off] = v
        out.update(kc=kc, kc_floor=fl, vc=vc)
    return out


def _emu_rot(x, cs_rows, neox, mutant):
    """x [T, nh, D] f32 rotated by cs_rows [T, D] in f32."""
    D = x.shape[-1]
    half = D // 2
    c, s = cs_rows[:, None, :half].float(), cs_rows[:, None, half:].float()
    if mutant == "swap_cs":
        c, s = s, c
    if mutant == "sin_sign":
        s = -s
    if mutant == "freq_shift":
        c, s = torch.roll(c, 8, -1), torch.roll(s, 8, -1)
    if neox != (mutant == "pairing"):
        x1, x2 = x[..., :half], x[..., half:]
        return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    x1, x2 = x[..., 0::2], x[..., 1::2]
    return torch.stack([x1 * c - x2 * s, x2 * c + x1 * s], -1).flatten(-2)


def emu_rope_kv(qkv, pos, cs, Hq, Hkv, D, kc=None, vc=None, slots=None, neox=True, write_k_inplace=False, mutant=None):
    """f32 CPU emulation of rope_kv_ on the given buffers (in place); ``mutant`` injects one fault."""
    T = qkv.shape[0]
    p = pos.long()
    if mutant == "neighbour_pos":
        p = torch.roll(p, 1)
    rows = cs[p]
    nq, nk = Hq * D, Hkv * D
    q = qkv[:, :nq].float().reshape(T, Hq, D)
    k = qkv[:, nq:nq + nk].float().reshape(T, Hkv, D)
    v = qkv[:, nq + nk:nq + 2 * nk].float().reshape(T, Hkv, D)
    qr, kr = _emu_rot(q, rows, neox, mutant).to(BF), _emu_rot(k, rows, neox, mutant).to(BF)
    qkv[:, :nq] = qr.reshape(T, nq)
    if write_k_inplace or mutant == "k_inplace_always":
        qkv[:, nq:nq + nk] = kr.reshape(T, nk)
    if kc is None:
        return
    NB, _, BS, _ = kc.shape
    sel, blk, off = slot_index(slots, BS)
    if mutant == "blk_off":
        blk, off = off % NB, blk % BS
    kw = k.to(BF) if mutant == "k_unrotated" else kr
    vw = _emu_rot(v, rows, neox, None).to(BF) if mutant == "v_rotated" else v.to(BF)
    if mutant == "cache_layout":  # [blk, off, h] instead of [blk, h, off]
        kc.view(NB, BS, Hkv, D)[blk, off] = kw[sel]
        vc.view(NB, BS, Hkv, D)[blk, off] = vw[sel]
    else:
        kc[blk, :, off] = kw[sel]
        vc[blk, :, off] = vw[sel]
    if mutant == "pad_to_slot0":
        for t, s in enumerate(slots):
            if s < 0:
                kc[0, :, 0] = kw[t]
                vc[0, :, 0] = vw[t]


def kv_want(k, v, slots, NB, BS):
    """Whole-cache answers of kv_write on SENTINEL caches (bitwise copies); ``slots`` a host list."""
    T, Hkv, D = k.shape
    sel, blk, off = slot_index(slots, BS, k.device)
    kc = torch.full((NB, Hkv, BS, D), SENTINEL, dtype=BF, device=k.device)
    vc = kc.clone()
    kc[blk, :, off] = k[sel]
    vc[blk, :, off] = v[sel]
    return kc, vc


# =============================================================================== activations
def all_bf16(device="cpu"):
    """Every one of the 65536 bf16 bit patterns, in pattern order."""
    return torch.arange(65536, dtype=torch.int32, device=device).to(torch.int16).view(BF)


def act_input(rows, N, device="cpu"):
    """[rows, N] bf16 walking the bit patterns cyclically (rows * N >= 65536: every pattern is there)."""
    assert rows * N >= 65536
    i = torch.arange(rows * N, device=device) % 65536
    return all_bf16(device)[i].reshape(rows, N)


def silu_input(rows, I, device="cpu"):
    """[rows, 2 I]: the gate walks the bit patterns; the up operand is 1 the first time a pattern
    comes up and walks UPS after that."""
    g = act_input(rows, I, device)
    n = torch.arange(rows * I, device=device)
    u = torch.tensor(UPS, device=device)[torch.where(n < 65536, torch.zeros_like(n), (n // 65536 + n % 65536 + n // 8) % 4)]
    return torch.cat([g, u.to(BF).reshape(rows, I)], dim=1)


def act_bias(N, device="cpu"):
    return torch.tensor(ACT_BIAS, dtype=torch.float64, device=device).repeat((N + 7) // 8)[:N].to(BF)


def silu_mul64(x):
    """-> (want, floor): g / (1 + exp(-g)) * u in float64."""
    I = x.shape[1] // 2
    g, u = x[:, :I].double(), x[:, I:].double()
    want = final64(G.silu64(g) * u)
    floor = torch.where(g.abs() < SUBNORMAL, torch.full_like(g, SUBNORMAL), torch.full_like(g, SILU_TINY)) * u.abs()
    return want, floor


def gelu_tanh64(e):
    return 0.5 * e * (1.0 + torch.tanh(0.7978845608028654 * (e + 0.044715 * e * e * e)))


def act64(x, bias, kind):
    """-> (want, floor, compared): kind 0 erf-GELU, 1 tanh-GELU, 2 ReLU of bf16(x + bias).  ReLU is
    compared bitwise (kind 'E'); its NaN inputs are left out of the comparison (fmaxf(NaN, 0) = 0
    where the float64 formula gives NaN): ``compared`` is False there and nowhere else."""
    e = x.double()
    if bias is not None:
        e = to_bf16(e + bias.double()[None, :])
    if kind == 2:
        keep = ~torch.isnan(e)
        return torch.where(keep, torch.relu(e), torch.zeros_like(e)), None, keep
    want = final64(G.gelu64(e) if kind == 0 else gelu_tanh64(e))
    fl = 0.5 * ERF_ABS * e.abs()
    return want, torch.where(torch.isfinite(fl), fl, torch.zeros_like(fl)), torch.ones_like(e, dtype=torch.bool)


def emu_silu_mul(x, mutant=None):
    I = x.shape[1] // 2
    g, u = x[:, :I].float(), x[:, I:].float()
    y = (g / (1.0 + torch.exp(-g))).to(BF).float() * u
    return round_store(y, mutant)


def round_store(y, mutant=None):
    """The kernels' f2bf of f32 values; mutant 'trunc': truncated instead of rounded."""
    if mutant == "trunc":
        return (y.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)
    return y.to(BF)


def emu_act(x, bias, kind, mutant=None):
    e = x.float()
    b = None if bias is None else bias.float()[None, :]
    if b is not None and mutant != "bias_after":
        e = round_store(e + b, mutant).float()
    if kind == 0 and mutant != "tanh_for_erf":
        y = G.emu_gelu(e)
    elif kind in (0, 1):
        y = 0.5 * e * (1.0 + torch.tanh(0.7978845608028654 * (e + 0.044715 * e * e * e)))
    else:
        y = torch.relu(e)
    if b is not None and mutant == "bias_after":
        y = y + b
    return round_store(y, mutant)


# =============================================================================== pooling, row norms
def pool_hidden(H, device="cpu", lens=POOL_LENS, pad=8):
    """-> (buf, hidden view [T, H] of integer-valued tokens with a row stride H + pad, cu int32)."""
    T = sum(lens)
    t = torch.arange(T, device=device)[:, None]
    c = torch.arange(H, device=device)[None, :]
    x = ((5 * t + 3 * c + t * c + c // 8) % 17 - 8).double()
    x[T - lens[-1]:] = 0.0  # the last sequence: all zeros
    cu = torch.tensor([sum(lens[:i]) for i in range(len(lens) + 1)], dtype=torch.int32, device=device)
    buf, view = in_padded(exact_bf16(x, "hidden"), pad)
    return buf, view, cu


def pool64(hidden, cu, mode, normalize):
    """float64 [B, H]; empty sequences and all-zero sequences give zeros."""
    cu = [int(v) for v in cu]
    H = hidden.shape[1]
    out = torch.zeros(len(cu) - 1, H, dtype=torch.float64, device=hidden.device)
    for b in range(len(cu) - 1):
        h = hidden[cu[b]:cu[b + 1]].double()
        if h.shape[0] == 0:
            continue
        v = h[0] if mode == 1 else h.sum(0) / h.shape[0]
        if normalize:
            v = v / max(float(v.pow(2).sum().sqrt()), 1e-12)
        out[b] = v
    return out


def emu_pool(hidden, cu, mode, normalize, mutant=None):
    cu = [int(v) for v in cu]
    T, H = hidden.shape
    out = torch.zeros(len(cu) - 1, H)
    for b in range(len(cu) - 1):
        beg, end = cu[b], cu[b + 1]
        n = end - beg
        if mode == 1:
            t0 = (end - 1) if mutant == "cls_last" else beg
            acc = hidden[t0].float() if n > 0 else torch.zeros(H)
        else:
            e2 = min(end + 1, T) if mutant == "next_seq" else end
            acc = hidden[beg:e2].float().sum(0)
            div = float(max(n, 1))
            if mutant == "n_plus_1":
                div = float(n + 1)
            if mutant == "div_h":
                div = float(H)
            acc = acc / div
        if normalize:
            nrm = torch.sqrt((acc * acc).sum())
            acc = acc * (1.0 / (nrm if mutant == "no_clamp" else nrm.clamp_min(1e-12)))
        out[b] = acc
    return out


def pool_bf16_floor(want):
    """A bf16 destination stores the f32 result rounded: half a bf16 ulp on top of the f32 bound."""
    return 0.5 * ulp_bf(want)


def square_rows(N, D, device="cpu"):
    """-> (x bf16 [N, D], norms f64 [N]): q = the largest m^2 with 2 m^2 <= D; row r holds q elements
    +-3 v and q elements +-4 v (v = r % 3 + 1) from column 8 r on (cyclic), the rest zero: the sum of
    squares is (5 m v)^2, exact in f32."""
    m = math.isqrt(D // 2)
    q = m * m
    r = torch.arange(N, device=device)[:, None]
    j = torch.arange(D, device=device)[None, :]
    v = (r % 3 + 1).double()
    vals = torch.where(j < 2 * q, torch.where(j % 2 == 0, 3 * v, 4 * v) * (1.0 - 2.0 * ((j // 3 + r) % 2).double()), torch.zeros((), dtype=torch.float64, device=device))
    x = torch.gather(vals.expand(N, D), 1, ((j - 8 * r) % D).expand(N, D))
    return exact_bf16(x, "x"), (5.0 * m * v).flatten()


# =============================================================================== argmax key
def key_rows(V, dtype, device="cpu"):
    """[B, V] logits for the key probes and the names of the rows.  Shards split the columns at
    shard_bounds(V, W); the rows are built so that the decisive columns sit in different shards."""
    b = shard_bounds(V, 3)
    c = torch.arange(V, device=device)
    neg = -1.0 - ((7 * c + 3) % 23).double()  # all negative, max -1 at several columns
    ninf = float("-inf")
    rows, names = [], []

    def add(name, row):
        names.append(name)
        rows.append(row)

    add("all negative", neg - 0.5 * (c == 0))
    tie = neg.clone()
    tie[[b[1] - 1, b[1] + 2, b[2] + 1]] = 4.0
    add("a tie across shards", tie)
    z = neg.clone()
    z[b[1] - 2], z[b[1] + 1], z[b[2]] = -0.0, 0.0, 0.0
    add("-0.0 in shard 0, +0.0 later", z)
    z = neg.clone()
    z[b[1] - 2], z[b[1] + 1], z[b[2]] = 0.0, -0.0, -0.0
    add("+0.0 in shard 0, -0.0 later", z)
    z = neg.clone()
    z[1], z[b[1]], z[V - 1] = -0.0, 0.0, 0.0
    add("-0.0 at id 1, +0.0 later", z)
    s = neg.clone()
    s[b[1]:b[2]] = ninf
    add("one shard all -inf", s)
    s = neg.clone()
    s[: b[1]] = ninf
    add("shard 0 all -inf", s)
    add("all -inf", torch.full((V,), ninf, dtype=torch.float64, device=device))
    n = neg.clone()
    n[[0, b[1], V - 1]] = float("nan")
    n[b[2] - 1] = 2.0
    add("NaN entries", n)
    n = neg.clone()
    n[b[1]:b[2]] = float("nan")
    add("one shard all NaN", n)
    last = neg.clone()
    last[V - 1] = 7.0
    add("the maximum in the last column", last)
    return torch.stack(rows).to(dtype), names


def shard_bounds(V, W):
    """Column bounds of W shards, none a multiple of 8 wide where V allows."""
    cut = [0] + [(V * i) // W + (3 if i else 0) for i in range(1, W)] + [V]
    return cut


def key_want(logits):
    """torch.argmax of the whole row with NaN as -inf (an all -inf row: id 0)."""
    x = logits.double()
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
    return x.argmax(-1).int()


def key_ids(logits, W, argmax_key, keys_to_ids):
    """The probe: split the columns into W shards (each a strided view of its own padded buffer),
    key every shard with its vocab_lo, stack and decode."""
    B, V = logits.shape
    cut = shard_bounds(V, W)
    keys = []
    for lo, hi in zip(cut[:-1], cut[1:]):
        w8 = (hi - lo + 7) // 8 * 8 + 16
        buf = torch.full((B, w8), 100.0, dtype=logits.dtype, device=logits.device)  # larger than any logit
        shard = buf[:, : hi - lo]
        shard.copy_(logits[:, lo:hi])
        keys.append(argmax_key(shard, lo))
    return keys_to_ids(torch.stack(keys))


# =============================================================================== the measurement
def _worst(kind, got, want, floor=None):
    x = excess(kind, got, want, floor)
    return float(x.max()) if x.numel() else 0.0


def measure_ulps():
    """Worst error of each emulation in ulps of the float64 answer over the domains named at ULPS."""
    out = dict.fromkeys(MEASURED, 0.0)
    for H in NORM_H:
        w, b = gamma(H), beta(H)
        x, _ = norm_rows(H)
        out["rms"] = max(out["rms"], _worst("rms", emu_rms(x, w), rms64(x, w)))
        xr, res = resid_rows(H)
        v = add64(xr, res)
        out["rms"] = max(out["rms"], _worst("rms", emu_rms(v, w), rms64(v, w)))
        xl, _ = ln_rows(H)
        tok, pos, typ = embed_tables(H)
        e = embed_sum(*embed_ids(), tok, pos, typ)
        for rows in (xl, v, e):
            for bb in (b, None):
                want, fl = ln64(rows, w, bb)
                out["ln"] = max(out["ln"], _worst("ln", emu_ln(rows, w, bb), want, fl))
    x = silu_input(4 * 8192, 8)
    for u in UPS:  # every gate against every up value
        xu = x.clone()
        xu[:, 8:] = u
        want, fl = silu_mul64(xu)
        out["silu"] = max(out["silu"], _worst("silu", emu_silu_mul(xu), want, fl))
    a = act_input(8192, 8)
    for kind, name in ((0, "gelu"), (1, "gelu_tanh")):
        for bias in (None, act_bias(8)):
            want, fl, _ = act64(a, bias, kind)
            out[name] = max(out[name], _worst(name, emu_act(a, bias, kind), want, fl))
    r = torch.arange(-32, 33, dtype=torch.float64)
    x1, x2 = r[:, None, None], r[None, :, None]
    for D in ROPE_D:
        cs = real_table(D)
        for p in ROPE_POS:
            c, s = cs[p, : D // 2], cs[p, D // 2:]
            y1, y2, f1, f2 = G.rotate64(x1, x2, c, s)
            e1, e2 = G.emu_rotate(x1, x2, c, s)
            out["rope"] = max(out["rope"], _worst("rope", e1.to(BF), y1, f1), _worst("rope", e2.to(BF), y2, f2))
    for H in POOL_H:
        _, hid, cu = pool_hidden(H)
        for mode in (0, 1):
            for nrm in (True, False):
                out["pool"] = max(out["pool"], _worst("pool", emu_pool(hid, cu, mode, nrm), pool64(hid, cu, mode, nrm)))
    return out
