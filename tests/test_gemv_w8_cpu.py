"""FP8 decode weights off the GPU: the row quantiser, the CPU reference of ops.gemv_decode_w8 (the
arithmetic of ops.gemv_decode on the dequantised weights), and the option from build_decoder through
the config and the command line to /api/show."""
import pytest
import torch
from fastapi.testclient import TestClient

from llm_kubernetes_minikube_sharp4dev_amd import ops
from llm_kubernetes_minikube_sharp4dev_amd.__main__ import _cfg
from llm_kubernetes_minikube_sharp4dev_amd.config import Config
from llm_kubernetes_minikube_sharp4dev_amd.models import build_decoder
from llm_kubernetes_minikube_sharp4dev_amd.parallel.tp import TPGroup
from llm_kubernetes_minikube_sharp4dev_amd.serving.model_manager import ModelManager
from llm_kubernetes_minikube_sharp4dev_amd.serving.ollama_server import create_app


def test_quantize_rows_e4m3():
    torch.manual_seed(0)
    w = (torch.randn(300, 1024) * torch.logspace(-3, 1, 300)[:, None]).to(torch.bfloat16)
    w[7] = 0
    w[8, 5:] = 0  # denormal codes next to one large value
    w[8, :5] = torch.tensor([3.0, 3.0 * 2 ** -9, 3.0 * 2 ** -8 * 1.4, -3.0 * 2 ** -12, 1e-30])
    wq, s = ops.quantize_rows_e4m3(w, block_rows=128)
    assert wq.dtype == torch.float8_e4m3fn and s.dtype == torch.float32 and s.shape == (300,)
    want_s = w.float().abs().amax(1) / 448
    want_s[7] = 1.0
    assert torch.equal(s, want_s)
    codes = wq.view(torch.uint8)
    assert not ((codes & 0x7F) == 0x7F).any(), "NaN encoding"
    assert not codes[7].any()
    q = wq.float()
    assert q.abs().max() == 448 and torch.equal(q.abs().amax(1)[s != 1], torch.full((299,), 448.0))
    err = (w.float() - q * s[:, None]).abs()
    assert (err <= s[:, None] * (2.0 ** -4 * q.abs() + 2.0 ** -10)).all()
    assert torch.equal(ops.dequantize_rows_e4m3(codes, s), q * s[:, None])


def test_reference_is_gemv_decode_on_dequantised_weights():
    torch.manual_seed(1)
    Hq, Hkv, D, BS, K = 4, 2, 32, 16, 1024
    N = (Hq + 2 * Hkv) * D
    x = torch.randn(2, K).to(torch.bfloat16)
    g = (torch.rand(K) + 0.5).to(torch.bfloat16)
    wq, s = ops.quantize_rows_e4m3((torch.randn(N, K) * 0.05).to(torch.bfloat16))
    wd = ops.dequantize_rows_e4m3(wq, s)
    assert torch.equal(ops.gemv_decode_w8(0, x, wq, s, g, 1e-5), ops.gemv_decode(0, x, wd, g, 1e-5))
    assert torch.equal(ops.gemv_decode_w8(0, x, wq.view(torch.uint8), s), ops.gemv_decode(0, x, wd))
    assert torch.equal(ops.gemv_decode_w8(2, x, wq, s, g, 1e-5), ops.gemv_decode(2, x, wd, g, 1e-5))
    res = torch.randn(2, N).to(torch.bfloat16)
    r1, r2 = res.clone(), res.clone()
    assert ops.gemv_decode_w8(1, x, wq, s, res=r1) is r1
    assert torch.equal(r1, ops.gemv_decode(1, x, wd, res=r2))
    kw = dict(positions=torch.tensor([17, 3], dtype=torch.int32), cos_sin=ops.rope_cos_sin(64, D, 10000.0), Hq=Hq,
              Hkv=Hkv, D=D, slots=torch.tensor([BS + 5, -1], dtype=torch.int32), neox=False)
    caches = [(torch.zeros(4, Hkv, BS, D, dtype=torch.bfloat16), torch.zeros(4, Hkv, BS, D, dtype=torch.bfloat16))
              for _ in range(2)]
    a = ops.gemv_decode_w8(3, x, wq, s, g, 1e-5, k_cache=caches[0][0], v_cache=caches[0][1], **kw)
    b = ops.gemv_decode(3, x, wd, g, 1e-5, k_cache=caches[1][0], v_cache=caches[1][1], **kw)
    assert torch.equal(a, b) and torch.equal(caches[0][0], caches[1][0]) and torch.equal(caches[0][1], caches[1][1])
    assert caches[0][0].abs().sum() > 0
    with pytest.raises(ValueError, match="K must be"):
        ops.gemv_decode_w8(0, x[:, :512], wq[:, :512].contiguous(), s)
    with pytest.raises(ValueError, match="M "):
        ops.gemv_decode_w8(0, torch.cat([x, x]), wq, s)


def test_build_decoder_decode_weights_values(monkeypatch):
    with pytest.raises(ValueError, match="decode_weights"):
        build_decoder("llama-tiny", decode_weights="int4")
    monkeypatch.setenv("LK_DECODE_WEIGHTS", "fp4")
    with pytest.raises(ValueError, match="decode_weights"):
        build_decoder("llama-tiny")
    monkeypatch.setenv("LK_DECODE_WEIGHTS", "fp8")
    with pytest.raises(ValueError, match="tensor parallel"):
        build_decoder("llama-tiny", tp=TPGroup(0, 2, None, None, [0, 1]))
    m = build_decoder("llama-tiny")  # the CPU keeps bf16 weights: the option is the GPU decode step's
    assert m.decode_weights == "bf16" and not hasattr(m.layers[0], "qkv_q")
    with pytest.raises(ValueError, match="tensor parallel"):
        build_decoder("llama-tiny", decode_weights="bf16", tp=TPGroup(0, 2, None, None, [0, 1])).quantize_decode_weights()


def test_quantize_decode_weights_buffers_and_reset():
    m = build_decoder("llama-tiny", decode_weights="bf16").quantize_decode_weights()
    L = m.layers[0]
    assert m.decode_weights == "fp8" and L.qkv_q.shape == L.qkv.shape and L.down_s.shape == (L.down.shape[0],)
    assert m.lm_head_q.shape == m.lm_head.shape and not any(k.endswith(("_q", "_s")) for k in m.state_dict())
    pad = m.lm_head_s[m.vocab_local:]
    assert torch.equal(pad, torch.ones_like(pad)) and not m.lm_head_q.view(torch.uint8)[m.vocab_local:].any()
    m.random_init(1)
    assert m.decode_weights == "bf16" and not hasattr(L, "qkv_q") and not hasattr(m, "lm_head_q")


@pytest.mark.parametrize("setting", ["bf16", "fp8"])
def test_config_cli_and_api_show(monkeypatch, setting):
    import argparse

    assert Config().engine.decode_weights == "bf16"
    monkeypatch.delenv("LK_ENGINE__DECODE_WEIGHTS", raising=False)
    cfg = _cfg(argparse.Namespace(config=None, decode_weights=setting))
    assert cfg.engine.decode_weights == setting
    assert _cfg(argparse.Namespace(config=None)).engine.decode_weights == setting  # (a child process: the environment)
    monkeypatch.delenv("LK_ENGINE__DECODE_WEIGHTS")
    mgr = ModelManager(cfg, device="cpu", aliases={"llama3.1:8b": "llama-tiny", "nomic-embed-text": "bert-tiny"})
    with TestClient(create_app(mgr)) as c:
        gen = c.post("/api/show", json={"model": "llama3.1:8b"}).json()
        emb = c.post("/api/show", json={"model": "nomic-embed-text"}).json()
    mgr.shutdown()
    base = ["format", "family", "families", "parameter_size", "quantization_level"]
    assert list(emb["details"]) == base
    assert list(gen["details"]) == base + (["decode_weights"] if setting == "fp8" else [])
    assert gen["details"].get("decode_weights") == (None if setting == "bf16" else "fp8_e4m3")
    assert list(gen) == ["modelfile", "parameters", "template", "details", "model_info", "capabilities"]
