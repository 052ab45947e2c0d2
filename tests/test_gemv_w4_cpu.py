"""MXFP4 decode weights off the GPU: the block quantiser, the CPU reference of ops.gemv_decode_w4 (the
arithmetic of ops.gemv_decode on the dequantised weights), and the option value from build_decoder
through the config and the command line to /api/show."""
import argparse

import pytest
import torch
from fastapi.testclient import TestClient

from llm_kubernetes_minikube_sharp4dev_amd import ops
from llm_kubernetes_minikube_sharp4dev_amd.__main__ import _cfg
from llm_kubernetes_minikube_sharp4dev_amd.models import build_decoder
from llm_kubernetes_minikube_sharp4dev_amd.parallel.tp import TPGroup
from llm_kubernetes_minikube_sharp4dev_amd.serving.model_manager import ModelManager
from llm_kubernetes_minikube_sharp4dev_amd.serving.ollama_server import create_app

BF = torch.bfloat16
GRID = torch.tensor(ops.E2M1_VALUES)


def test_quantize_rows_mxfp4():
    torch.manual_seed(0)
    w = (torch.randn(40, 256) * torch.logspace(-3, 1, 40)[:, None]).to(BF)
    w[7, 32:64] = 0                                            # an all-zero block
    w[8, :32] = 3.0 * 2.0 ** -12                               # tiny values beside one large one
    w[8, 5] = 3.0
    mids = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    w[9, :32] = 0
    w[9, :16] = torch.cat([torch.tensor([6.0]), mids, -mids, torch.tensor([7.5])]) * 2.0 ** -5  # exact ties; (6, 8)
    wq4, wexp = ops.quantize_rows_mxfp4(w, block_rows=16)
    assert wq4.dtype == wexp.dtype == torch.uint8 and wq4.shape == (40, 128) and wexp.shape == (40, 8)
    assert wq4.is_contiguous() and wexp.is_contiguous() and not (wexp == 0xFF).any()
    blk = w.float().view(40, 8, 32)
    amax = blk.abs().amax(2)
    want_e = (torch.floor(torch.log2(amax.double())) - 2 + 127).clamp(1, 254)
    want_e[amax == 0] = 127
    assert torch.equal(wexp.double(), want_e) and wexp[7, 1] == 127 and wexp[9, 0] == 122
    # unpacked by hand: weight 2 j in the low nibble of byte j, weight 2 j + 1 in the high nibble
    code = torch.stack((wq4 & 0xF, wq4 >> 4), 2).view(40, 256).long()
    q = GRID[code & 7] * (1 - 2 * (code >> 3)).float()
    scale = torch.exp2(wexp.float() - 127)[:, :, None]
    deq = ops.dequantize_rows_mxfp4(wq4, wexp)
    assert torch.equal(deq, (q.view(40, 8, 32) * scale).view(40, 256))
    assert not code[7, 32:64].any() and torch.equal(deq[8, :8], torch.tensor([0, 0, 0, 0, 0, 3.0, 0, 0]))
    even = torch.tensor([0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0])   # nearest even at each midpoint
    assert torch.equal(deq[9, :16] * 32, torch.cat([torch.tensor([6.0]), even, -even, torch.tensor([6.0])]))
    # half a grid step at that magnitude (0.5 below 2, 1 below 4, 2 above), or the clamp in (6, 8)
    v = (blk / scale).abs()
    half = torch.where(v > 6, v - 6, torch.where(v >= 4, 1.0, torch.where(v >= 2, 0.5, 0.25)))
    assert v.max() < 8 and ((deq.view(40, 8, 32) - blk).abs() <= half * scale).all()


def _grid(N, K, seed, exps=(-8, -7)):
    """bf16 w = q * 2^e, q on the e2m1 grid with one |q| of 4 or 6 per block of 32, e per block: the
    OCP rule recovers e and quantize_rows_mxfp4 is exact."""
    g = torch.Generator().manual_seed(seed)
    code = torch.randint(0, 16, (N, K // 32, 32), generator=g)
    code[:, :, 0] = torch.randint(6, 8, (N, K // 32), generator=g) + 8 * torch.randint(0, 2, (N, K // 32), generator=g)
    code = torch.gather(code, 2, torch.rand(N, K // 32, 32, generator=g).argsort(2))  # (the large one anywhere)
    e = torch.tensor(exps)[torch.randint(0, len(exps), (N, K // 32), generator=g)]
    return (GRID[code & 7] * (1 - 2 * (code >> 3)).float() * torch.exp2(e.float())[:, :, None]).view(N, K).to(BF)


def test_reference_is_gemv_decode_on_dequantised_weights():
    torch.manual_seed(1)
    Hq, Hkv, D, BS, K = 4, 2, 32, 16, 2048
    N = (Hq + 2 * Hkv) * D
    x = torch.randn(2, K).to(BF)
    g = (torch.rand(K) + 0.5).to(BF)
    w = _grid(N, K, 3)
    wq4, wexp = ops.quantize_rows_mxfp4(w)
    wd = ops.dequantize_rows_mxfp4(wq4, wexp)
    assert torch.equal(wd, w.float()), "the grid must round-trip"
    assert torch.equal(ops.gemv_decode_w4(0, x, wq4, wexp, g, 1e-5), ops.gemv_decode(0, x, wd, g, 1e-5))
    assert torch.equal(ops.gemv_decode_w4(2, x, wq4, wexp, g, 1e-5), ops.gemv_decode(2, x, wd, g, 1e-5))
    res = torch.randn(2, N).to(BF)
    r1, r2 = res.clone(), res.clone()
    assert ops.gemv_decode_w4(1, x, wq4, wexp, res=r1) is r1
    assert torch.equal(r1, ops.gemv_decode(1, x, wd, res=r2))
    kw = dict(positions=torch.tensor([17, 3], dtype=torch.int32), cos_sin=ops.rope_cos_sin(64, D, 10000.0), Hq=Hq,
              Hkv=Hkv, D=D, slots=torch.tensor([BS + 5, -1], dtype=torch.int32), neox=False)
    caches = [(torch.zeros(4, Hkv, BS, D, dtype=BF), torch.zeros(4, Hkv, BS, D, dtype=BF)) for _ in range(2)]
    a = ops.gemv_decode_w4(3, x, wq4, wexp, g, 1e-5, k_cache=caches[0][0], v_cache=caches[0][1], **kw)
    b = ops.gemv_decode(3, x, wd, g, 1e-5, k_cache=caches[1][0], v_cache=caches[1][1], **kw)
    assert torch.equal(a, b) and torch.equal(caches[0][0], caches[1][0]) and torch.equal(caches[0][1], caches[1][1])
    assert caches[0][0].abs().sum() > 0
    with pytest.raises(ValueError, match="K must be"):
        ops.gemv_decode_w4(0, x[:, :1024], wq4[:, :512].contiguous(), wexp[:, :32].contiguous())
    with pytest.raises(ValueError, match="M "):
        ops.gemv_decode_w4(0, torch.cat([x, x[:1]]), wq4, wexp)


def test_quantize_decode_weights_kinds_and_reset(monkeypatch):
    m = build_decoder("llama-tiny", decode_weights="mxfp4")  # the CPU keeps bf16 weights
    L = m.layers[0]
    assert m.decode_weights == "bf16" and not hasattr(L, "qkv_q4")
    m.quantize_decode_weights("mxfp4")
    assert m.decode_weights == "mxfp4" and not hasattr(L, "qkv_q") and not hasattr(m, "lm_head_q")
    for name in ("qkv", "o", "gate_up", "down"):
        n, k = getattr(L, name).shape
        assert getattr(L, name + "_q4").shape == (n, k // 2) and getattr(L, name + "_e").shape == (n, k // 32)
    assert m.lm_head_q4.shape == (m.lm_head.shape[0], m.lm_head.shape[1] // 2)
    assert not any(k.endswith(("_q4", "_e")) for k in m.state_dict())
    assert not m.lm_head_q4[m.vocab_local:].any() and (m.lm_head_e[m.vocab_local:] == 127).all()
    m.quantize_decode_weights()
    assert m.decode_weights == "fp8" and hasattr(L, "qkv_q") and not hasattr(L, "qkv_q4") and not hasattr(m, "lm_head_e")
    m.quantize_decode_weights("mxfp4")
    assert m.decode_weights == "mxfp4" and not hasattr(L, "qkv_s")
    m.random_init(1)
    assert m.decode_weights == "bf16" and not hasattr(L, "qkv_q4") and not hasattr(m, "lm_head_q4")
    with pytest.raises(ValueError, match="kind"):
        m.quantize_decode_weights("int4")
    monkeypatch.setenv("LK_DECODE_WEIGHTS", "mxfp4")
    with pytest.raises(ValueError, match="tensor parallel"):
        build_decoder("llama-tiny", tp=TPGroup(0, 2, None, None, [0, 1]))


def test_config_cli_and_api_show(monkeypatch):
    monkeypatch.setenv("LK_ENGINE__DECODE_WEIGHTS", "bf16")  # (registered: teardown restores today's state)
    monkeypatch.delenv("LK_ENGINE__DECODE_WEIGHTS")
    cfg = _cfg(argparse.Namespace(config=None, decode_weights="mxfp4"))
    assert cfg.engine.decode_weights == "mxfp4"
    assert _cfg(argparse.Namespace(config=None)).engine.decode_weights == "mxfp4"  # (a child process: the environment)
    monkeypatch.delenv("LK_ENGINE__DECODE_WEIGHTS")
    mgr = ModelManager(cfg, device="cpu", aliases={"llama3.1:8b": "llama-tiny", "nomic-embed-text": "bert-tiny"})
    with TestClient(create_app(mgr)) as c:
        gen = c.post("/api/show", json={"model": "llama3.1:8b"}).json()
        emb = c.post("/api/show", json={"model": "nomic-embed-text"}).json()
    mgr.shutdown()
    base = ["format", "family", "families", "parameter_size", "quantization_level"]
    assert list(emb["details"]) == base and list(gen["details"]) == base + ["decode_weights"]
    assert gen["details"]["decode_weights"] == "mxfp4_e2m1"
