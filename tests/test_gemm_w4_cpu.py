"""MXFP4 decode GEMM off the GPU: ops.gemm_decode_w4 is ops.gemv_decode's reference arithmetic on the
dequantised weights for 3 to 16 rows, its limits are ValueErrors, and the GEMV keeps its own."""
import pytest
import torch

from llm_kubernetes_minikube_sharp4dev_amd import ops

BF = torch.bfloat16


def _operands(M, N, K):
    torch.manual_seed(N + K)
    wq4, wexp = ops.quantize_rows_mxfp4((torch.randn(N, K) * 0.02).to(BF))
    return torch.randn(M, K).to(BF), wq4, wexp


def test_reference_row_by_row():
    Hq, Hkv, D, BS, K = 2, 1, 32, 16, 2048
    N = (Hq + 2 * Hkv) * D
    x, wq4, wexp = _operands(3, N, K)
    wd = ops.dequantize_rows_mxfp4(wq4, wexp)
    g = (torch.rand(K) + 0.5).to(BF)
    res = torch.randn(3, N).to(BF)
    pos, slots = torch.tensor([17, 3, 40], dtype=torch.int32), torch.tensor([BS + 5, -1, 2], dtype=torch.int32)
    cs = ops.rope_cos_sin(64, D, 10000.0)
    kc, vc = torch.zeros(4, Hkv, BS, D, dtype=BF), torch.zeros(4, Hkv, BS, D, dtype=BF)
    r3 = res.clone()
    got = [ops.gemm_decode_w4(0, x, wq4, wexp, g, 1e-5), ops.gemm_decode_w4(2, x, wq4, wexp, g, 1e-5),
           ops.gemm_decode_w4(1, x, wq4, wexp, res=r3),
           ops.gemm_decode_w4(3, x, wq4, wexp, g, 1e-5, positions=pos, cos_sin=cs, Hq=Hq, Hkv=Hkv, D=D, k_cache=kc,
                              v_cache=vc, slots=slots, neox=False)]
    assert got[2] is r3 and kc.abs().sum() > 0
    for m in range(3):  # one row at a time through the GEMV's reference
        xm, k1, v1 = x[m:m + 1], torch.zeros_like(kc), torch.zeros_like(vc)
        want = [ops.gemv_decode(0, xm, wd, g, 1e-5), ops.gemv_decode(2, xm, wd, g, 1e-5),
                ops.gemv_decode(1, xm, wd, res=res[m:m + 1].clone()),
                ops.gemv_decode(3, xm, wd, g, 1e-5, positions=pos[m:m + 1], cos_sin=cs, Hq=Hq, Hkv=Hkv, D=D, k_cache=k1,
                                v_cache=v1, slots=slots[m:m + 1], neox=False)]
        for a, b in zip(got, want):
            assert torch.equal(a[m:m + 1], b)
        if slots[m] >= 0:
            blk, off = slots[m] // BS, slots[m] % BS
            assert torch.equal(kc[blk, :, off], k1[blk, :, off]) and torch.equal(vc[blk, :, off], v1[blk, :, off])


@pytest.mark.parametrize("M,N,K,name", [(2, 32, 256, "M "), (17, 32, 256, "M "), (3, 32, 384, "K must"),
                                        (3, 48, 256, "N must")])
def test_value_errors(M, N, K, name):
    with pytest.raises(ValueError, match=name):
        ops.gemm_decode_w4(0, *_operands(M, N, K))


def test_gemv_still_refuses_three_rows():
    x, wq4, wexp = _operands(3, 32, 2048)
    with pytest.raises(ValueError, match="M "):
        ops.gemv_decode_w4(0, x, wq4, wexp)
