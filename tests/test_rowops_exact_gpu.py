"""The row-wise kernels against the structured probes of tests/row_probes.py, whose float64 answers
pin every element: the norms (csrc/norm.hip) over every ROW_DISPATCH arm and its edges, RoPE + the
paged KV write and kv_write (csrc/rope_kv.hip), the activations over every bf16 bit pattern
(csrc/activation.hip), pooling and row norms (csrc/pooling.hip) and the vocab-parallel argmax key
(csrc/sampling.hip).  Every output and in-place buffer is larger than the result and filled with
SENTINEL; the answers cover the whole buffer.  tests/test_row_probes_cpu.py shows what these
comparisons reject."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import row_probes as R  # noqa: E402
from test_gemm_exact_gpu import Checks  # noqa: E402

from llm_kubernetes_minikube_sharp4dev_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
EPS = R.NORM_EPS


class _Detail:
    """The name of a comparison; formatted only when it failed: then with the first wrong element."""

    def __init__(self, what, kind, got, want, floor):
        self.args = (kind, got, want, floor, what)

    def __format__(self, spec):
        return R.describe(*self.args)

    __str__ = lambda self: format(self)  # noqa: E731


class RowChecks(Checks):
    """Checks (counted on the device, one read-back in finish()) under the rules of row_probes: a
    comparison enters as its boolean verdict per element, which must be all False."""

    def near(self, kind, got, want, what, floor=None):
        verdict = R.bad(kind, got, want, floor)
        self.add("E", verdict, torch.zeros_like(verdict), _Detail(what, kind, got, want, floor))

    def same(self, got, want, what):
        """Bitwise-equal values of whole buffers (bf16 / f32 / int against the exact answer)."""
        self.near("E", got, want, what)


def _raises_before_launch(fn):
    with pytest.raises(RuntimeError):
        fn()


# ================================================================ RMSNorm
@pytest.mark.parametrize("H", R.NORM_H)
def test_rmsnorm(hip, H):
    """Spike, dense, all-zero and eps-dominated rows, plain and into a strided ``out`` from a strided
    ``x``; residual sums with exact ties from a strided residual (updated bit-exact)."""
    w = R.gamma(H, DEV)
    x, _ = R.norm_rows(H, DEV)
    want = R.rms64(x, w)
    ck = RowChecks()
    ck.near("rms", ops.rmsnorm(x, w, EPS), want, f"rmsnorm H{H}")
    xbuf, xv = R.in_padded(x, 16)
    obuf, ov = R.padded(x.shape[0], H, DEV, pad_cols=24)
    keep = xbuf.clone()
    out = ops.rmsnorm(xv, w, EPS, None, ov)
    assert out.data_ptr() == ov.data_ptr()
    ck.near("rms", obuf, R.want_padded(want, obuf), f"rmsnorm H{H} strided x, out=")
    ck.same(xbuf, keep, f"rmsnorm H{H}: x is not written")
    xr, res = R.resid_rows(H, DEV)
    new = R.add64(xr, res)
    xbuf, xv = R.in_padded(xr, 8)
    for given_out in (False, True):
        rbuf, rv = R.in_padded(res, 16)
        obuf, ov = R.padded(xr.shape[0], H, DEV, pad_cols=24)
        out = ops.rmsnorm(xv, w, EPS, rv, ov if given_out else None)
        ck.same(rbuf, R.want_padded(new, rbuf), f"rmsnorm H{H}: the residual stream (out= {given_out})")
        if given_out:
            ck.near("rms", obuf, R.want_padded(R.rms64(new, w), obuf), f"rmsnorm H{H} + residual, out=")
        else:
            ck.near("rms", out, R.rms64(new, w), f"rmsnorm H{H} + residual")
    ck.finish()


@pytest.mark.parametrize("H", [16392, 12])
def test_norms_refuse_unsupported_widths(hip, H):
    x = torch.zeros(2, H, dtype=BF, device=DEV)
    w = torch.ones(H, dtype=BF, device=DEV)
    _raises_before_launch(lambda: ops.rmsnorm(x, w, EPS))
    _raises_before_launch(lambda: ops.layernorm(x, w, w, EPS))
    ids = torch.zeros(2, dtype=torch.int32, device=DEV)
    _raises_before_launch(lambda: ops.embed_layernorm(ids, None, None, x, None, None, w, w, EPS))
    torch.cuda.synchronize()


# ================================================================ LayerNorm
def _ln_checks(ck, out, v, w, b, nconst, what):
    want, fl = R.ln64(v, w, b)
    ck.near("ln", out, want, what, floor=fl)
    if nconst is not None:  # zero variance: the bias bit for bit (0 without one)
        ck.same(out[nconst:nconst + 2], want[nconst:nconst + 2], what + ": constant rows")


@pytest.mark.parametrize("H", R.NORM_H)
def test_layernorm(hip, H):
    """Spike rows, constant rows, mean 256 with small deviations, dense rows; with and without a
    bias, strided rows, a residual that is read only and one that is written back."""
    w, b = R.gamma(H, DEV), R.beta(H, DEV)
    x, nc = R.ln_rows(H, DEV)
    ck = RowChecks()
    xbuf, xv = R.in_padded(x, 16)
    keep = xbuf.clone()
    for bb in (b, None):
        _ln_checks(ck, ops.layernorm(x, w, bb, EPS), x, w, bb, nc, f"layernorm H{H} bias {bb is not None}")
        _ln_checks(ck, ops.layernorm(xv, w, bb, EPS), x, w, bb, nc, f"layernorm H{H} strided bias {bb is not None}")
    ck.same(xbuf, keep, f"layernorm H{H}: x is not written")
    xr, res = R.resid_rows(H, DEV)
    new = R.add64(xr, res)
    _, xv = R.in_padded(xr, 8)
    for write in (False, True):
        for bb in (b, None):
            rbuf, rv = R.in_padded(res, 24)
            keep = rbuf.clone()
            out = ops.layernorm(xv, w, bb, EPS, residual=rv, write_residual=write)
            what = f"layernorm H{H} residual, write {write}, bias {bb is not None}"
            _ln_checks(ck, out, new, w, bb, None, what)
            ck.same(rbuf, R.want_padded(new, rbuf) if write else keep, what + ": the residual buffer")
    ck.finish()


@pytest.mark.parametrize("H", R.NORM_H)
def test_embed_layernorm(hip, H):
    """All tables; no type table; a type table without type_ids (row 0); no position table.  Ids 0 and
    V - 1; token V - 1 at position 0, type 0 sums to a constant: the bias bit for bit."""
    w, b = R.gamma(H, DEV), R.beta(H, DEV)
    tok, pos, typ = R.embed_tables(H, DEV)
    ids, pid, yid = R.embed_ids(device=DEV)
    ck = RowChecks()
    for name, a in (("all tables", (ids, pid, yid, tok, pos, typ)), ("no type table", (ids, pid, None, tok, pos, None)),
                    ("no type_ids", (ids, pid, None, tok, pos, typ)), ("no position table", (ids, None, yid, tok, None, typ)),
                    ("token table only", (ids, None, None, tok, None, None))):
        out = ops.embed_layernorm(*a, w, b, EPS)
        want, fl = R.ln64(R.embed_sum(*a), w, b)
        ck.near("ln", out, want, f"embed_layernorm H{H} {name}", floor=fl)
        if name in ("all tables", "no type_ids"):
            ck.same(out[1], b, f"embed_layernorm H{H} {name}: the constant row")
    ck.finish()


# ================================================================ RoPE + KV write
HEADS = [(1, 1), (4, 4), (5, 1), (32, 8)]


def _positions(T, real):
    p = [R.ROPE_POS[(t + 1) % 4] for t in range(T)] if real else [(7 * t + 2) % R.ROPE_MAX_POS for t in range(T)]
    return torch.tensor(p, dtype=torch.int32, device=DEV)


def _rope_case(ck, cs, real, neox, D, Hq, Hkv, T, BS, wki, caches, what):
    NB = 3 if BS >= 8 else 12
    pos = _positions(T, real)
    buf, qkv = R.qkv_rows(T, Hq, Hkv, D, DEV, pad=8 if (T + BS) % 2 else 24)
    slots = R.slot_list(T, NB, BS) if caches else None
    want = R.rope_want(qkv.clone(), buf, pos, cs, Hq, Hkv, D, neox, wki, NB, BS, slots)
    kc = vc = st = None
    if caches:
        kc = torch.full((NB, Hkv, BS, D), R.SENTINEL, dtype=BF, device=DEV)
        vc = kc.clone()
        st = torch.tensor(slots, dtype=torch.int32, device=DEV)
    ops.rope_kv_(qkv, pos, cs, Hq, Hkv, D, kc, vc, st, neox, wki)
    if real:
        ck.near("rope", buf, want["row"], what + ": qkv", floor=want["row_floor"])
    else:
        ck.same(buf, want["row"], what + ": qkv")
    if caches:
        if real:
            ck.near("rope", kc, want["kc"], what + ": k cache", floor=want["kc_floor"])
        else:
            ck.same(kc, want["kc"], what + ": k cache")
        ck.same(vc, want["vc"], what + ": v cache")


@pytest.mark.parametrize("D", R.ROPE_D)
@pytest.mark.parametrize("neox", [True, False])
def test_rope_kv_exact(hip, neox, D):
    """The synthetic table ({0, +-0.5, +-1}) on small integers: every buffer bit for bit -- q rotated,
    k rotated in the row only with write_k_inplace, v and the row padding untouched, rotated k and raw
    v at their slots, every other cache row still the sentinel; with and without caches."""
    cs = R.synth_table(R.ROPE_MAX_POS, D, DEV)
    ck = RowChecks()
    for Hq, Hkv in HEADS:
        for T in (1, 3, 5):
            for wki in (True, False):
                for BS in (1, 8, 16, 128):
                    _rope_case(ck, cs, False, neox, D, Hq, Hkv, T, BS, wki, True, f"rope_kv neox {neox} D{D} heads {Hq}/{Hkv} T{T} BS{BS} wki {wki}")
                _rope_case(ck, cs, False, neox, D, Hq, Hkv, T, 1, wki, False, f"rope_kv neox {neox} D{D} heads {Hq}/{Hkv} T{T} wki {wki} no caches")
        ck.finish()


@pytest.mark.parametrize("D", R.ROPE_D)
@pytest.mark.parametrize("neox", [True, False])
def test_rope_kv_real_table(hip, neox, D):
    """ref.rope_cos_sin(theta 500000) at positions {0, 1, 37, max_pos - 1}: position 0 returns the input
    (its float64 answer is the input and its floor 0 up to 4 * 2^-24 |x|), the others within ULPS['rope']."""
    cs = ops.rope_cos_sin(R.ROPE_MAX_POS, D, theta=R.ROPE_THETA, device=DEV)
    ck = RowChecks()
    for Hq, Hkv in HEADS:
        for T, BS, wki in ((1, 16, False), (3, 8, True), (5, 16, False), (5, 128, True)):
            _rope_case(ck, cs, True, neox, D, Hq, Hkv, T, BS, wki, True, f"rope_kv real neox {neox} D{D} heads {Hq}/{Hkv} T{T} BS{BS} wki {wki}")
        # position 0 alone: bit for bit the input
        buf, qkv = R.qkv_rows(3, Hq, Hkv, D, DEV)
        keep = buf.clone()
        ops.rope_kv_(qkv, torch.zeros(3, dtype=torch.int32, device=DEV), cs, Hq, Hkv, D, None, None, None, neox, True)
        ck.same(buf, keep, f"rope_kv real neox {neox} D{D} heads {Hq}/{Hkv}: position 0")
    ck.finish()


def test_rope_kv_refuses_d24(hip):
    cs = R.synth_table(8, 24, DEV)
    _, qkv = R.qkv_rows(2, 2, 1, 24, DEV)
    _raises_before_launch(lambda: ops.rope_kv_(qkv, torch.zeros(2, dtype=torch.int32, device=DEV), cs, 2, 1, 24))
    torch.cuda.synchronize()


def _kv_inputs(T, Hkv, D, pad=8):
    """k and v as strided views into one packed [T, 3 Hkv D + pad] buffer."""
    buf, qkv = R.qkv_rows(T, Hkv, Hkv, D, DEV, pad)
    n = Hkv * D
    return buf, qkv[:, n:2 * n].view(T, Hkv, D), qkv[:, 2 * n:3 * n].view(T, Hkv, D)


@pytest.mark.parametrize("Hkv,D", [(2, 64), (8, 128), (9, 128), (4, 256)])
def test_kv_write(hip, Hkv, D):
    """Hkv * D / 8 below, equal to and above the 128 threads; T 1 and 4 with a -1 slot; the caches start
    as SENTINEL and are compared whole, bit for bit; the source is not written."""
    ck = RowChecks()
    for T, NB, BS in ((1, 3, 16), (4, 3, 16), (4, 12, 1), (5, 2, 128)):
        buf, k, v = _kv_inputs(T, Hkv, D)
        keep = buf.clone()
        slots = R.slot_list(T, NB, BS)
        kc = torch.full((NB, Hkv, BS, D), R.SENTINEL, dtype=BF, device=DEV)
        vc = kc.clone()
        ops.kv_write(k, v, kc, vc, torch.tensor(slots, dtype=torch.int32, device=DEV))
        wk, wv = R.kv_want(k, v, slots, NB, BS)
        what = f"kv_write Hkv{Hkv} D{D} T{T} BS{BS}"
        ck.same(kc, wk, what + ": k cache")
        ck.same(vc, wv, what + ": v cache")
        ck.same(buf, keep, what + ": the source")
    ck.finish()


def test_kv_write_refuses_bad_arguments(hip):
    T, Hkv, D, NB, BS = 4, 2, 64, 3, 16
    _, k, v = _kv_inputs(T, Hkv, D)
    kc = torch.full((NB, Hkv, BS, D), R.SENTINEL, dtype=BF, device=DEV)
    vc = kc.clone()
    sl = torch.tensor([0, 5, -1, 47, 9, 3, 2, 1], dtype=torch.int32, device=DEV)
    _raises_before_launch(lambda: ops.kv_write(k, v, kc, vc, sl[:3]))       # one slot per token
    _raises_before_launch(lambda: ops.kv_write(k, v, kc, vc, sl))
    _raises_before_launch(lambda: ops.kv_write(k, v, kc, vc, sl[::2]))      # contiguous slots
    _raises_before_launch(lambda: ops.kv_write(k, v, kc, vc, sl[:4].cpu()))  # everything on the device
    _raises_before_launch(lambda: ops.kv_write(k, v, kc.cpu(), vc, sl[:4]))
    _raises_before_launch(lambda: ops.kv_write(k, v, kc, vc.cpu(), sl[:4]))
    _raises_before_launch(lambda: ops.kv_write(k, v, kc, vc[:2], sl[:4]))   # the caches agree
    torch.cuda.synchronize()
    assert bool((kc == R.SENTINEL).all()) and bool((vc == R.SENTINEL).all())


# ================================================================ activations
ACT_SHAPES = [(65540, 8, 0), (16, 4104, 8), (37, 1792, 24)]  # rows past the 65535 grid rows; strided rows


@pytest.mark.parametrize("rows,I,pad", ACT_SHAPES)
def test_silu_mul_every_bit_pattern(hip, rows, I, pad):
    """Every bf16 bit pattern as the gate (up = 1 the first time, then {-2, 0.5, 3}): finite gates
    within ULPS['silu'], +-inf, NaN and subnormal gates as the float64 formula g / (1 + exp(-g)) has it."""
    x = R.silu_input(rows, I, DEV)
    want, fl = R.silu_mul64(x)
    ck = RowChecks()
    if pad:
        xbuf, xv = R.in_padded(x, pad)
        obuf, ov = R.padded(rows, I, DEV, pad_cols=pad + 8)
        ops.silu_mul(xv, ov)
        ck.near("silu", obuf, R.want_padded(want, obuf), f"silu_mul {rows} x {I} strided", floor=R.want_padded(fl, obuf).clamp_min(0))
    else:
        ck.near("silu", ops.silu_mul(x), want, f"silu_mul {rows} x {I}", floor=fl)
    ck.finish()


@pytest.mark.parametrize("rows,N,pad", ACT_SHAPES)
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_activation_every_bit_pattern(hip, kind, rows, N, pad):
    """In-place act(x + bias), kinds erf-GELU, tanh-GELU and ReLU, without a bias and with one whose
    sums hold exact bf16 ties.  ReLU is bit-exact on every input that is not NaN (the kernel's
    fmaxf(NaN, 0) is 0, the float64 formula keeps NaN: those inputs are left out)."""
    a = R.act_input(rows, N, DEV)
    name = ("gelu", "gelu_tanh", "relu")[kind]
    ck = RowChecks()
    for bias in (None, R.act_bias(N, DEV)):
        want, fl, keep = R.act64(a, bias, kind)
        buf, x = R.in_padded(a, pad) if pad else (None, a.clone())
        hip.activation_(x, bias, kind)
        what = f"activation {name} {rows} x {N} bias {bias is not None}"
        if kind == 2:
            ck.same(torch.where(keep, x.double(), torch.zeros_like(want)), want, what)
        else:
            ck.near(name, x, want, what, floor=fl)
        if pad:
            ck.same(buf[:, N:], torch.full_like(buf[:, N:], R.SENTINEL), what + ": row padding")
            ck.same(buf[rows:], torch.full_like(buf[rows:], R.SENTINEL), what + ": rows beyond")
    ck.finish()


# ================================================================ pooling, row norms
@pytest.mark.parametrize("H", R.POOL_H)
def test_pool_normalize(hip, H):
    """Sequence lengths [3, 0, 1, 40, 0, 2 (all zeros)], a hidden row stride above H, f32 and bf16
    destinations that are strided slices of a sentinel buffer; empty and all-zero sequences give
    zeros; CLS without normalisation is a copy."""
    hbuf, hid, cu = R.pool_hidden(H, DEV)
    keep = hbuf.clone()
    B = cu.numel() - 1
    ck = RowChecks()
    for mode in (0, 1):
        for nrm in (True, False):
            want = R.pool64(hid, cu, mode, nrm)
            what = f"pool_normalize H{H} mode {mode} normalize {nrm}"
            ck.near("pool", ops.pool_normalize(hid, cu, mode, nrm), want, what)
            for dt in (torch.float32, BF):
                obuf, ov = R.padded(B, H, DEV, dtype=dt, pad_cols=16)
                out = ops.pool_normalize(hid, cu, mode, nrm, out=ov)
                assert out.data_ptr() == ov.data_ptr()
                full = R.want_padded(want, obuf)
                if mode == 1 and not nrm:
                    ck.same(obuf, full, what + f" {dt}: a copy")
                else:
                    ck.near("pool", obuf, full, what + f" {dt}", floor=R.pool_bf16_floor(full) if dt == BF else None)
    ck.same(hbuf, keep, f"pool_normalize H{H}: hidden is not written")
    ck.finish()


def test_pool_normalize_refuses_h4104(hip):
    _, hid, cu = R.pool_hidden(4104, DEV)
    _raises_before_launch(lambda: ops.pool_normalize(hid, cu, 0, True))
    torch.cuda.synchronize()


def test_pool_reference_matches_the_kernel_on_empty_sequences(hip):
    """ops.reference.pool_normalize is the CPU path of ops.pool_normalize: the same zeros."""
    _, hid, cu = R.pool_hidden(768, DEV)
    ck = RowChecks()
    for mode in (0, 1):
        for nrm in (True, False):
            got = ops.pool_normalize(hid, cu, mode, nrm)
            cpu = ops.pool_normalize(hid.cpu(), cu.cpu(), mode, nrm)
            assert cpu.shape == got.shape and bool(torch.isfinite(cpu).all())
            ck.same(got[[1, 4, 5]], cpu[[1, 4, 5]].to(DEV), f"mode {mode} normalize {nrm}: the empty and the all-zero sequences")
    ck.finish()


@pytest.mark.parametrize("D", [8, 512, 520, 1032])
def test_row_norms(hip, D):
    """Integer rows whose sum of squares is a perfect square (exact in f32): within 1 f32 ulp."""
    ck = RowChecks()
    for N in (1, 5, 9):
        x, nrm = R.square_rows(N, D, DEV)
        ck.near("rownorm", ops.row_norms(x), nrm, f"row_norms N{N} D{D}")
    ck.finish()


# ================================================================ argmax key
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [50, 1003, 2600])
def test_argmax_key_across_shards(hip, dtype, V):
    """keys_to_ids over the argmax_key of 1, 2 and 3 column shards (each a strided view, widths no
    multiple of 8) equals torch.argmax of the whole row: ties and +-0.0 across shards take the lowest
    global id, an all -inf shard loses, an all -inf row gives id 0, NaN counts as -inf."""
    logits, names = R.key_rows(V, dtype, DEV)
    want = R.key_want(logits)
    ck = RowChecks()
    for W in (1, 2, 3):
        got = R.key_ids(logits, W, ops.argmax_key, ops.key_to_id)
        assert got.dtype == torch.int32
        ck.same(got, want, f"argmax key V{V} {dtype} W{W} (rows: {names})")
    ck.finish()
