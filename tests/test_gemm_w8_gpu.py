"""FP8 decode GEMM for 3 to 16 rows (csrc/gemm_decode_w8.hip): exact probes compared bit for bit, every
mode against fp64 of the dequantised weights on a grid the quantiser round-trips, the refusals, and one
5-row decode step of a small Llama on the FP8 copies against the same model on bf16.

Worst errors measured on an MI355X (bound in brackets): see docs/decode_fp8_rows.md."""
import functools

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


def _close(a, b, atol, rtol, msg):
    a, b = a.double().cpu(), b.double().cpu()
    err, tol = (a - b).abs().max().item(), atol + rtol * b.abs().max().item()
    print(f"{msg}: max abs err {err:.4g} (bound {tol:.4g})")
    assert err <= tol, f"{msg} max abs err {err:.4g} > {tol:.4g}"


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16).cpu(), b.contiguous().view(torch.int16).cpu())


# ------------------------------------------------------------------ 1. exact probes
@functools.lru_cache(maxsize=None)
def _probe(K, pattern, NM=96, MM=16):
    """(wq [NM, K] e4m3, wscale [NM], x [MM, K] at row stride K + 8, y64 [MM, NM]): integer weights in
    -8 .. 8, x integers in -2 .. 2, row scale 2^-(3 + n % 4): every sum is a multiple of 2^-6 below
    2^18, exact in fp32 in any order."""
    k, n = np.arange(K), np.arange(NM)
    x = np.stack([((k + 3 * m) % 5) - 2 for m in range(MM)]).astype(np.int64)
    if pattern == "dense":
        q = np.random.default_rng(K).integers(-8, 9, size=(NM, K), dtype=np.int64)
    else:  # row n: one non-zero at column (7 n + 3) % K; magnitude and sign depend on n
        q = np.zeros((NM, K), np.int64)
        q[n, (7 * n + 3) % K] = (1 + n % 8) * np.where(n % 3 == 0, -1, 1)
    s = 2.0 ** -(3 + n % 4)
    xs = torch.zeros(MM, K + 8, device=DEV, dtype=BF)
    xs[:, :K] = torch.from_numpy(x.astype(np.float32)).to(BF)
    return (torch.from_numpy(q.astype(np.float32)).to(torch.float8_e4m3fn).to(DEV),
            torch.from_numpy(s.astype(np.float32)).to(DEV), xs[:, :K], torch.from_numpy((x @ q.T) * s[None, :]))


@pytest.mark.parametrize("pattern", ["dense", "onehot"])
@pytest.mark.parametrize("N", [32, 96])
@pytest.mark.parametrize("K", [256, 2048, 14336])
@pytest.mark.parametrize("M", [3, 5, 16])
def test_exact_probes(hip, M, K, N, pattern):
    wq, ws, xv, y64 = _probe(K, pattern)
    r64 = torch.from_numpy(((np.arange(M)[:, None] * 7 + np.arange(N)[None, :]) % 9 - 4).astype(np.float64))
    assert xv[:M].stride(0) == K + 8
    want0 = y64[:M, :N].float().to(BF)
    want1 = (want0.float() + r64.float()).to(BF)
    for _ in range(2):
        assert _bits(ops.gemm_decode_w8(0, xv[:M], wq[:N], ws[:N]), want0), "mode 0"
        res = r64.to(BF).to(DEV)
        out = ops.gemm_decode_w8(1, xv[:M], wq[:N], ws[:N], res=res)
        assert out.data_ptr() == res.data_ptr() and _bits(res, want1), "mode 1"


# ------------------------------------------------------------------ 2. every mode vs fp64, lossless grid
def _grid(N, K, seed, exps=(-13, -12)):
    """bf16 w = q * 2^e with q on the e4m3 grid and one |q| = 448 per row: quantize_rows_e4m3 is exact."""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 256, (N, K), generator=g, dtype=torch.uint8)
    codes = torch.where((codes & 0x7F) == 0x7F, codes - 1, codes)  # (no NaN codes)
    q = codes.view(torch.float8_e4m3fn).float()
    q[torch.arange(N), torch.randint(0, K, (N,), generator=g)] = 448.0 * (1 - 2 * torch.randint(0, 2, (N,), generator=g))
    e = torch.tensor(exps)[torch.randint(0, len(exps), (N,), generator=g)]
    return (q * torch.exp2(e.float())[:, None]).to(BF)


def _quantised(w):
    wq, s = ops.quantize_rows_e4m3(w)
    assert torch.equal(ops.dequantize_rows_e4m3(wq, s), w.float()), "the grid must round-trip"
    return wq.to(DEV), s.to(DEV)


def _normed(x, g, eps):
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return ((xf * inv).to(BF).float() * g.float()).to(BF)


# (5, 768): the last LDS-DMA instruction of a staged row is half a wave
@pytest.mark.parametrize("M,K", [(3, 2048), (16, 2048), (3, 14336), (16, 14336), (5, 768)])
def test_modes_vs_fp64(hip, M, K):
    torch.manual_seed(K + M)
    Hq, Hkv, D, BS = 2, 1, 128, 16
    N = (Hq + 2 * Hkv) * D
    w = _grid(N, K, K + M)
    wq, ws = _quantised(w)
    x = torch.randn(M, K, dtype=BF)
    g = (torch.rand(K) + 0.5).to(BF)
    res = torch.randn(M, N, dtype=BF)
    xd = x.to(DEV)
    norm = M * (2 * K + 16) + 2 * K <= 159 * 1024  # the RMSNorm prologue's X image fits in LDS
    assert norm == ((M, K) != (16, 14336))
    gd = g.to(DEV) if norm else None
    lin = x.double() @ w.double().t()
    lin_n = _normed(x, g, 1e-5).double() @ w.double().t() if norm else lin
    _close(hip.gemm_decode_w8(0, xd, wq, ws), lin, 0.02, 0.01, f"plain M{M} K{K}")
    if norm:
        _close(hip.gemm_decode_w8(0, xd, wq, ws, gd, 1e-5), lin_n, 0.02, 0.01, f"plain + norm M{M} K{K}")
    rd = res.to(DEV)
    hip.gemm_decode_w8(1, xd, wq, ws, res=rd)
    _close(rd, (lin.to(BF).double() + res.double()).to(BF), 0.03, 0.01, f"residual M{M} K{K}")
    _close(hip.gemm_decode_w8(2, xd, wq, ws, gd, 1e-5), ref.silu_mul(lin_n.to(BF)), 0.03, 0.01,
           f"swiglu norm {norm} M{M} K{K}")
    cos_sin = ops.rope_cos_sin(4096, D, 500000.0, None, device="cpu")
    pos = (torch.arange(M, dtype=torch.int32) * 211 + 37) % 4096
    slots = (torch.arange(M, dtype=torch.int32) * 9 + 3).int()
    slots[1] = -1
    for neox in (True, False):
        kc = torch.zeros(12, Hkv, BS, D, device=DEV, dtype=BF)
        vc = torch.zeros_like(kc)
        kc_ref, vc_ref = kc.cpu(), vc.cpu()
        unrot = lin_n.to(BF)
        qkv_ref = ref.rope_kv_(unrot.clone(), pos, cos_sin, Hq, Hkv, D, kc_ref, vc_ref, slots, neox, False)
        qkv = hip.gemm_decode_w8(3, xd, wq, ws, gd, 1e-5, None, pos.to(DEV), cos_sin.to(DEV), Hq, Hkv, D, kc, vc,
                                 slots.to(DEV), neox)
        what = f"norm {norm} M{M} K{K} neox {neox}"
        _close(qkv[:, : Hq * D], qkv_ref[:, : Hq * D], 0.03, 0.01, "q rotated " + what)
        _close(qkv[:, Hq * D:], unrot[:, Hq * D:], 0.03, 0.01, "k / v rows (k unrotated) " + what)
        _close(kc, kc_ref, 0.03, 0.01, "k cache " + what)
        _close(vc, vc_ref, 0.03, 0.01, "v cache " + what)
        written = (M - 1) * Hkv * D  # slot -1: unwritten
        assert torch.count_nonzero(kc.float()) == written and torch.count_nonzero(vc.float()) == written


# ------------------------------------------------------------------ 3. refusals
def _case(name):
    """(mode, x, wq, wscale, kwargs) breaking one limit."""
    M, N, K = {"M \\(rows": (17, 32, 256), "M must": (2, 32, 256), "K must": (3, 32, 384), "N must": (3, 48, 256),
               "LDS": (16, 32, 14336)}.get(name, (4, 128, 256))
    x = torch.zeros(M, K, device=DEV, dtype=BF)
    wq = torch.zeros(N, K, device=DEV, dtype=torch.uint8)
    ws = torch.ones(N, device=DEV)
    mode, kw = 0, {}
    if name == "M must":
        name = "M \\(rows"
    elif name == "LDS":
        kw = dict(gamma=torch.ones(K, device=DEV, dtype=BF))
    elif name == "ldx":
        x = torch.zeros(M, K + 4, device=DEV, dtype=BF)[:, :K]
    elif name == "x must be 16-byte":
        x = torch.zeros(M * K + 4, device=DEV, dtype=BF)[4:].view(M, K)
    elif name == "x must be bfloat16":
        x = x.half()
    elif name == "wq must be 16-byte":
        wq = torch.zeros(N * K + 1, device=DEV, dtype=torch.uint8)[1:].view(N, K)
    elif name == "wq must be contiguous":
        wq = wq.to(torch.int8)
    elif name == "x must be \\[M, K\\]":
        wq = torch.zeros(N, 2 * K, device=DEV, dtype=torch.uint8)
    elif name == "wscale must be":
        ws = ws.double()
    elif name in ("mode 3 needs", "D a multiple"):  # N != (Hq + 2 Hkv) D; D % 32
        mode, D = 3, 32 if name == "mode 3 needs" else 16
        kw = dict(positions=torch.zeros(M, device=DEV, dtype=torch.int32), slots=torch.zeros(M, device=DEV, dtype=torch.int32),
                  cos_sin=torch.zeros(8, D, device=DEV), Hq=1 if D == 32 else 4, Hkv=1 if D == 32 else 2, D=D)
    elif name == "mode 1 needs res":
        mode, kw = 1, dict(res=torch.zeros(M, N + 2, device=DEV, dtype=BF)[:, :N])
    return name, mode, x, wq, ws, kw


@pytest.mark.parametrize("name", ["M \\(rows", "M must", "K must", "N must", "LDS", "ldx", "x must be 16-byte",
                                  "x must be bfloat16", "wq must be 16-byte", "wq must be contiguous",
                                  "x must be \\[M, K\\]", "wscale must be", "mode 3 needs", "D a multiple",
                                  "mode 1 needs res"])
def test_refusals(hip, name):
    name, mode, x, wq, ws, kw = _case(name)
    with pytest.raises(ValueError, match=name):
        ops.gemm_decode_w8(mode, x, wq, ws, **kw)
    with pytest.raises(RuntimeError):
        hip.gemm_decode_w8(mode, x, wq, ws, **kw)
    wq, ws, xv, y64 = _probe(256, "dense")
    assert _bits(hip.gemm_decode_w8(0, xv[:3], wq, ws), y64[:3].float().to(BF))


# ------------------------------------------------------------------ 4. one decode step
def test_decode_step_fp8_equals_bf16(hip):
    cfg = DecoderConfig("w8-rows", "llama", num_layers=2, hidden=2048, num_heads=16, num_kv_heads=4, head_dim=128,
                        intermediate=4096, vocab_size=1000, max_position=256)
    m = LlamaModel(cfg, device=DEV).random_init(0).eval()
    seed = 0
    for L in m.layers:
        for p in (L.qkv, L.o, L.gate_up, L.down):
            seed += 1
            p.copy_(_grid(p.shape[0], p.shape[1], seed).to(DEV))
        L.input_norm.copy_((torch.rand(2048) + 0.5).to(BF))
        L.post_norm.copy_((torch.rand(2048) + 0.5).to(BF))
    m.lm_head[: m.vocab_local].copy_(_grid(m.vocab_local, 2048, 99).to(DEV))
    M, BS = 5, 16
    pos = torch.tensor([20, 9, 31, 0, 17], dtype=torch.int32, device=DEV)
    bt = torch.arange(1, 11, dtype=torch.int32, device=DEV).view(5, 2)
    slots = (bt.gather(1, (pos // BS).long()[:, None])[:, 0] * BS + pos % BS).int()
    torch.manual_seed(5)
    kv0 = [(torch.randn(12, 4, BS, 128, device=DEV).to(BF), torch.randn(12, 4, BS, 128, device=DEV).to(BF)) for _ in range(2)]
    ids = torch.tensor([5, 777, 31, 2, 640], dtype=torch.int32, device=DEV)
    outs = {}
    for arm in ("fp8", "bf16"):
        meta = AttnMeta(positions=pos, slots=slots, num_decode=M, block_tables_d=bt, ctx_lens_d=pos + 1)
        kv = [(k.clone(), v.clone()) for k, v in kv0]
        if arm == "fp8":
            m.quantize_decode_weights("fp8")
        else:
            m.drop_decode_weights()
        steps = m.gemm_w8_steps
        h = m.forward(ids, meta, kv)
        assert m.decode_weights == arm and m.gemm_w8_steps - steps == (arm == "fp8") and m.gemm_w4_steps == 0
        outs[arm] = (h, kv, m.head(h))
    _close(outs["fp8"][0], outs["bf16"][0], 0.06, 0.02, "final hidden")
    _close(outs["fp8"][2], outs["bf16"][2], 0.06, 0.02, "logits")
    assert outs["fp8"][2].shape == (M, 1000)
    for (k1, v1), (k2, v2), (k0, _) in zip(outs["fp8"][1], outs["bf16"][1], kv0):
        _close(k1, k2, 0.05, 0.01, "k cache")
        _close(v1, v2, 0.05, 0.01, "v cache")
        assert not torch.equal(k1, k0)
