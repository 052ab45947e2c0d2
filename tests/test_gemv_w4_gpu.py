"""MXFP4 decode GEMV (csrc/gemv_decode_mxfp4.hip): exact probes compared bit for bit, every mode against
fp64 of the dequantised weights on a grid the quantiser round-trips, the refusals, and one decode
step of a small Llama on the MXFP4 copies against the same model on its bf16 weights.

Worst errors measured on an MI355X (bound in brackets): see docs/decode_mxfp4.md."""
import numpy as np
import pytest
import torch

from llm_kubernetes_minikube_sharp4dev_amd import ops
from llm_kubernetes_minikube_sharp4dev_amd.models.attention import AttnMeta
from llm_kubernetes_minikube_sharp4dev_amd.models.configs import DecoderConfig
from llm_kubernetes_minikube_sharp4dev_amd.models.llama import LlamaModel
from llm_kubernetes_minikube_sharp4dev_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
GRID = torch.tensor(ops.E2M1_VALUES)


def _close(a, b, atol, rtol, msg):
    a, b = a.double().cpu(), b.double().cpu()
    err, tol = (a - b).abs().max().item(), atol + rtol * b.abs().max().item()
    print(f"{msg}: max abs err {err:.4g} (bound {tol:.4g})")
    assert err <= tol, f"{msg} max abs err {err:.4g} > {tol:.4g}"


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16).cpu(), b.contiguous().view(torch.int16).cpu())


# ------------------------------------------------------------------ 1. exact probes
def _probe(K, pattern, NM=520):
    """(wq4 [NM, K/2], wexp [NM, K/32], x [2, K] at row stride K + 8, y64 [2, NM]): weights from
    {0, +-1, +-2, +-3, +-4, +-6} times block scales 2^-3 .. 2^0, x integers in -2 .. 2: every sum is
    a multiple of 2^-3 below 2^21, exact in fp32 in any order."""
    k, n = np.arange(K), np.arange(NM)
    x = np.stack([((k + 3 * m) % 5) - 2 for m in range(2)]).astype(np.int64)
    mags = np.array([0, 1, 2, 3, 4, 6])
    if pattern == "dense":
        rng = np.random.default_rng(K)
        q = mags[rng.integers(0, 6, size=(NM, K))] * rng.choice([-1, 1], size=(NM, K))
    else:  # row n: one non-zero at column (7 n + 3) % K; magnitude, sign and block scale depend on n
        q = np.zeros((NM, K), np.int64)
        q[n, (7 * n + 3) % K] = mags[1 + n % 5] * np.where(n % 3 == 0, -1, 1)
    e = -((n[:, None] + 3 * np.arange(K // 32)[None, :]) % 4)  # per block: 0 .. -3
    y = x @ (q * 2 ** (e.repeat(32, axis=1) + 3)).T  # in eighths
    code = np.array([0, 2, 4, 5, 6, 0, 7])[np.abs(q)] + 8 * (q < 0)
    wq4 = (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8)
    xs = torch.zeros(2, K + 8, device=DEV, dtype=BF)
    xs[:, :K] = torch.from_numpy(x.astype(np.float32)).to(BF)
    return (torch.from_numpy(wq4).to(DEV), torch.from_numpy((e + 127).astype(np.uint8)).to(DEV), xs[:, :K],
            torch.from_numpy(y.astype(np.float64) / 8))


@pytest.mark.parametrize("pattern", ["dense", "onehot"])
@pytest.mark.parametrize("K", [2048, 4096, 14336])
def test_exact_probes(hip, K, pattern):
    wq4, wexp, xv, y64 = _probe(K, pattern)
    r64 = torch.from_numpy(((np.arange(2)[:, None] * 7 + np.arange(520)[None, :]) % 9 - 4).astype(np.float64))
    for N in (2, 10, 520):
        for M in (1, 2):
            what = f"K{K} N{N} M{M} {pattern}"
            assert hip.gemv_w4_supported(M, N, K, 0) and xv[:M].stride(0) == K + 8
            want0 = y64[:M, :N].float().to(BF)
            outs = [ops.gemv_decode_w4(0, xv[:M], wq4[:N], wexp[:N]) for _ in range(2)]
            assert _bits(outs[0], want0) and _bits(outs[1], want0), what + " mode 0"
            want1 = (want0.float() + r64[:M, :N].float()).to(BF)
            for _ in range(2):
                res = r64[:M, :N].to(BF).to(DEV)
                out = ops.gemv_decode_w4(1, xv[:M], wq4[:N], wexp[:N], res=res)
                assert out.data_ptr() == res.data_ptr() and _bits(res, want1), what + " mode 1"


# ------------------------------------------------------------------ 2. every mode vs fp64, lossless grid
def _grid(N, K, seed, exps=(-8, -7)):
    """bf16 w = q * 2^e, q on the e2m1 grid with one |q| of 4 or 6 per block of 32, e per block: the
    OCP rule recovers e and quantize_rows_mxfp4 is exact."""
    g = torch.Generator().manual_seed(seed)
    code = torch.randint(0, 16, (N, K // 32, 32), generator=g)
    code[:, :, 0] = torch.randint(6, 8, (N, K // 32), generator=g) + 8 * torch.randint(0, 2, (N, K // 32), generator=g)
    code = torch.gather(code, 2, torch.rand(N, K // 32, 32, generator=g).argsort(2))  # (the large one anywhere)
    e = torch.tensor(exps)[torch.randint(0, len(exps), (N, K // 32), generator=g)]
    return (GRID[code & 7] * (1 - 2 * (code >> 3)).float() * torch.exp2(e.float())[:, :, None]).view(N, K).to(BF)


def _quantised(w):
    wq4, wexp = ops.quantize_rows_mxfp4(w)
    assert torch.equal(ops.dequantize_rows_mxfp4(wq4, wexp), w.float()), "the grid must round-trip"
    return wq4.to(DEV), wexp.to(DEV)


def _normed(x, g, eps):
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return ((xf * inv).to(BF).float() * g.float()).to(BF)


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("K", [2048, 14336])
def test_modes_vs_fp64(hip, M, K):
    torch.manual_seed(K + M)
    Hq, Hkv, D, BS = 2, 1, 128, 16
    N = (Hq + 2 * Hkv) * D
    w = _grid(N, K, K + M)
    wq4, we = _quantised(w)
    x = torch.randn(M, K, dtype=BF)
    g = (torch.rand(K) + 0.5).to(BF)
    res = torch.randn(M, N, dtype=BF)
    xd, gd = x.to(DEV), g.to(DEV)
    lin = x.double() @ w.double().t()
    lin_n = _normed(x, g, 1e-5).double() @ w.double().t()
    _close(hip.gemv_decode_w4(0, xd, wq4, we), lin, 0.02, 0.01, f"plain M{M} K{K}")
    _close(hip.gemv_decode_w4(0, xd, wq4, we, gd, 1e-5), lin_n, 0.02, 0.01, f"plain + norm M{M} K{K}")
    rd = res.to(DEV)
    hip.gemv_decode_w4(1, xd, wq4, we, res=rd)
    _close(rd, (lin.to(BF).double() + res.double()).to(BF), 0.03, 0.01, f"residual M{M} K{K}")
    _close(hip.gemv_decode_w4(2, xd, wq4, we, gd, 1e-5), ref.silu_mul(lin_n.to(BF)), 0.03, 0.01, f"swiglu M{M} K{K}")
    cos_sin = ops.rope_cos_sin(4096, D, 500000.0, None, device="cpu")
    pos = torch.tensor([37, 2049][:M], dtype=torch.int32)
    slots = torch.tensor([5 * BS + 3, -1][:M], dtype=torch.int32)
    for neox in (True, False):
        kc = torch.zeros(12, Hkv, BS, D, device=DEV, dtype=BF)
        vc = torch.zeros_like(kc)
        kc_ref, vc_ref = kc.cpu(), vc.cpu()
        unrot = lin_n.to(BF)
        qkv_ref = ref.rope_kv_(unrot.clone(), pos, cos_sin, Hq, Hkv, D, kc_ref, vc_ref, slots, neox, False)
        qkv = hip.gemv_decode_w4(3, xd, wq4, we, gd, 1e-5, None, pos.to(DEV), cos_sin.to(DEV), Hq, Hkv, D, kc, vc,
                                 slots.to(DEV), neox)
        what = f"M{M} K{K} neox {neox}"
        _close(qkv[:, : Hq * D], qkv_ref[:, : Hq * D], 0.03, 0.01, "q rotated " + what)
        _close(qkv[:, Hq * D:], unrot[:, Hq * D:], 0.03, 0.01, "k / v rows (k unrotated) " + what)
        _close(kc, kc_ref, 0.03, 0.01, "k cache " + what)
        _close(vc, vc_ref, 0.03, 0.01, "v cache " + what)
        assert torch.count_nonzero(kc.float()) == Hkv * D and torch.count_nonzero(vc.float()) == Hkv * D  # slot -1: unwritten


# ------------------------------------------------------------------ 3. refusals
def _case(name):
    """(x, wq4, wexp, kwargs) breaking one limit."""
    M, N, K = {"M ": (3, 4, 2048), "K must": (1, 4, 3072), "N must": (1, 3, 2048), "LDS": (2, 4, 28672)}.get(name, (2, 4, 2048))
    x = torch.zeros(M, K, device=DEV, dtype=BF)
    wq4 = torch.zeros(N, K // 2, device=DEV, dtype=torch.uint8)
    wexp = torch.full((N, K // 32), 127, device=DEV, dtype=torch.uint8)
    kw = {}
    if name == "ldx":
        x = torch.zeros(M, K + 4, device=DEV, dtype=BF)[:, :K]
    elif name == "x must be 16-byte":
        x = torch.zeros(K + 4, device=DEV, dtype=BF)[4:].view(1, K)
    elif name == "wq4 must be 16-byte":
        wq4 = torch.zeros(N * K // 2 + 1, device=DEV, dtype=torch.uint8)[1:].view(N, K // 2)
    elif name == "wq4 must be contiguous uint8":
        wq4 = torch.zeros(N, K, device=DEV, dtype=torch.uint8)
    elif name == "wexp must":
        wexp = wexp.float()
    elif name == "mode 3":
        kw = dict(positions=torch.zeros(M, device=DEV, dtype=torch.int32), slots=torch.zeros(M, device=DEV, dtype=torch.int32),
                  cos_sin=torch.zeros(8, 2, device=DEV), Hq=1, Hkv=1, D=2)  # N != (Hq + 2 Hkv) D
    return x, wq4, wexp, kw


@pytest.mark.parametrize("name", ["M ", "K must", "N must", "LDS", "ldx", "x must be 16-byte", "wq4 must be 16-byte",
                                  "wq4 must be contiguous uint8", "wexp must", "mode 3"])
def test_refusals(hip, name):
    x, wq4, wexp, kw = _case(name)
    mode = 3 if name == "mode 3" else 0
    with pytest.raises(ValueError, match=name):
        ops.gemv_decode_w4(mode, x, wq4, wexp, **kw)
    with pytest.raises(RuntimeError):
        hip.gemv_decode_w4(mode, x, wq4, wexp, **kw)
    wq4, wexp, xv, y64 = _probe(2048, "dense", 10)
    assert _bits(hip.gemv_decode_w4(0, xv, wq4, wexp), y64.float().to(BF))


# ------------------------------------------------------------------ 4. one decode step
@pytest.mark.parametrize("folded", [False, True])
def test_decode_step_mxfp4_equals_bf16(hip, folded):
    cfg = DecoderConfig("w4-step", "llama", num_layers=2, hidden=2048, num_heads=16, num_kv_heads=4, head_dim=128,
                        intermediate=4096, vocab_size=1000, max_position=256)
    m = LlamaModel(cfg, device=DEV).random_init(0).eval()
    seed = 0
    for L in m.layers:
        for p in (L.qkv, L.o, L.gate_up, L.down):
            seed += 1
            p.copy_(_grid(p.shape[0], p.shape[1], seed).to(DEV))
    m.lm_head[: m.vocab_local].copy_(_grid(m.vocab_local, 2048, 99).to(DEV))
    torch.manual_seed(5)
    if folded:
        m.fold_norms()  # (norm weights of 1: the permuted rows stay on the grid)
    else:
        for L in m.layers:
            L.input_norm.copy_((torch.rand(2048) + 0.5).to(BF))
            L.post_norm.copy_((torch.rand(2048) + 0.5).to(BF))
    M, BS = 2, 16
    pos = torch.tensor([20, 9], dtype=torch.int32, device=DEV)
    bt = torch.tensor([[1, 2], [3, 4]], dtype=torch.int32, device=DEV)
    slots = (bt.gather(1, (pos // BS).long()[:, None])[:, 0] * BS + pos % BS).int()
    kv0 = [(torch.randn(6, 4, BS, 128, device=DEV).to(BF), torch.randn(6, 4, BS, 128, device=DEV).to(BF)) for _ in range(2)]
    ids = torch.tensor([5, 777], dtype=torch.int32, device=DEV)
    outs = {}
    for arm in ("mxfp4", "bf16"):
        meta = AttnMeta(positions=pos, slots=slots, num_decode=M, block_tables_d=bt, ctx_lens_d=pos + 1)
        kv = [(k.clone(), v.clone()) for k, v in kv0]
        if arm == "mxfp4":
            m.quantize_decode_weights("mxfp4")
            for L in m.layers:
                assert torch.equal(ops.dequantize_rows_mxfp4(L.down_q4, L.down_e), L.down.float())
            assert m._w4_ok(M)
        else:
            m.drop_decode_weights()
            assert not m._w4_ok(M)
        assert m.decode_weights == arm and m._gemv_ok(m.embed_tokens(ids), meta)
        h = m._forward_decode_gemv(m.embed_tokens(ids), meta, kv)
        outs[arm] = (h, kv, m.head(h))
    _close(outs["mxfp4"][0], outs["bf16"][0], 0.06, 0.02, f"final hidden folded {folded}")
    _close(outs["mxfp4"][2], outs["bf16"][2], 0.06, 0.02, f"logits folded {folded}")
    assert outs["mxfp4"][2].shape == (M, 1000)
    for (k1, v1), (k2, v2), (k0, _) in zip(outs["mxfp4"][1], outs["bf16"][1], kv0):
        _close(k1, k2, 0.05, 0.01, "k cache")
        _close(v1, v2, 0.05, 0.01, "v cache")
        assert not torch.equal(k1, k0)
