"""FP8 decode GEMM off the GPU: ops.gemm_decode_w8 is ops.gemv_decode's reference arithmetic on the
dequantised weights for 3 to 16 rows, 2 and 17 rows are ValueErrors, and a CPU model never routes."""
import pytest
import torch

from llm_kubernetes_minikube_sharp4dev_amd import ops
from llm_kubernetes_minikube_sharp4dev_amd.models.attention import AttnMeta
from llm_kubernetes_minikube_sharp4dev_amd.models.configs import DecoderConfig
from llm_kubernetes_minikube_sharp4dev_amd.models.llama import LlamaModel

BF = torch.bfloat16


def _operands(M, N, K):
    torch.manual_seed(N + K)
    wq, ws = ops.quantize_rows_e4m3((torch.randn(N, K) * 0.02).to(BF))
    return torch.randn(M, K).to(BF), wq, ws


def test_reference_on_dequantised_weights():
    Hq, Hkv, D, BS, K = 2, 1, 32, 16, 256
    N = (Hq + 2 * Hkv) * D
    x, wq, ws = _operands(3, N, K)
    wd = ops.dequantize_rows_e4m3(wq, ws)
    g = (torch.rand(K) + 0.5).to(BF)
    res = torch.randn(3, N).to(BF)
    rope = dict(positions=torch.tensor([17, 3, 40], dtype=torch.int32), cos_sin=ops.rope_cos_sin(64, D, 10000.0), Hq=Hq,
                Hkv=Hkv, D=D, slots=torch.tensor([BS + 5, -1, 2], dtype=torch.int32), neox=False)
    caches = [torch.zeros(4, Hkv, BS, D, dtype=BF) for _ in range(4)]
    r1, r2 = res.clone(), res.clone()
    got = [ops.gemm_decode_w8(0, x, wq, ws, g, 1e-5), ops.gemm_decode_w8(1, x, wq, ws, res=r1),
           ops.gemm_decode_w8(2, x, wq, ws, g, 1e-5),
           ops.gemm_decode_w8(3, x, wq, ws, g, 1e-5, k_cache=caches[0], v_cache=caches[1], **rope)]
    want = [ops.gemv_decode(0, x, wd, g, 1e-5), ops.gemv_decode(1, x, wd, res=r2), ops.gemv_decode(2, x, wd, g, 1e-5),
            ops.gemv_decode(3, x, wd, g, 1e-5, k_cache=caches[2], v_cache=caches[3], **rope)]
    assert got[1] is r1 and caches[0].abs().sum() > 0
    for a, b in zip(got + caches[:2], want + caches[2:]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("M", [2, 17])
def test_rows_outside_3_to_16(M):
    with pytest.raises(ValueError, match="M "):
        ops.gemm_decode_w8(0, *_operands(M, 32, 256))


def test_cpu_model_is_not_routed():
    cfg = DecoderConfig("w8-rows-cpu", "llama", num_layers=1, hidden=256, num_heads=2, num_kv_heads=1, head_dim=128,
                        intermediate=256, vocab_size=64, max_position=64)
    m = LlamaModel(cfg, device="cpu").random_init(0).eval().quantize_decode_weights("fp8")
    pos = torch.arange(5, dtype=torch.int32)
    meta = AttnMeta(positions=pos, slots=pos, num_decode=5)
    assert m.decode_weights == "fp8" and m.gemm_w8_steps == 0
    assert not m._gemm_w8_ok(torch.zeros(5, 256, dtype=BF), meta)
