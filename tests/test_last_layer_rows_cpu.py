"""The last decoder block on the logit rows only (LK_LAST_LAYER_ROWS) against the block on every
row, through ``_forward_chain`` on the CPU reference ops: the step shapes of
tests/test_last_layer_rows_gpu.py, exact equality of the returned hidden rows and of the whole
KV cache, and the reference forms of the two new ops."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import last_layer_steps as S  # noqa: E402

from llm_kubernetes_minikube_sharp4dev_amd import ops  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.models import llama as llama_mod  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.ops import reference as R  # noqa: E402


@pytest.fixture(scope="module")
def model():
    return S.build_model("cpu", torch.bfloat16)


def _mm_by_row(x, w):
    """x w^T one row at a time: the library's fp32 GEMM sums a row in an order that depends on how
    many rows it is given, which is exactly what differs between the two runs compared here (the
    HIP kernel's order does not: tests/test_last_layer_rows_gpu.py)."""
    wt = w.float().t().contiguous()
    xf = x.float()
    return torch.cat([xf[i:i + 1] @ wt for i in range(xf.shape[0])]) if xf.shape[0] else xf @ wt


def _run(model, monkeypatch, on, shape, follow=False):
    monkeypatch.setattr(llama_mod, "LAST_LAYER_ROWS", on)
    monkeypatch.setattr(R, "_mm", _mm_by_row)
    runner = S.new_runner(model)
    items = shape(S.StepMaker())
    before = model.last_layer_rows
    h, meta = S.run_chain(model, runner, items)
    took = model.last_layer_rows - before
    h2 = None
    if follow:
        si, _ = runner.prepare(S.follow_up(items))
        ids, meta2 = runner._meta(si)
        with torch.inference_mode():
            h2 = model(ids, meta2, runner.kv_caches)
    return h, runner.kv.clone(), took, meta, h2


@pytest.mark.parametrize("shape,rows,pruned", [(S.mixed_333, 6, True), (S.two_tiles, 131, True),
                                               (S.no_logit_rows, 0, False), (S.many_logit_rows, 200, False)])
def test_switch_on_equals_switch_off(model, monkeypatch, shape, rows, pruned):
    follow = shape is S.mixed_333
    h1, kv1, took1, meta, f1 = _run(model, monkeypatch, True, shape, follow)
    h0, kv0, took0, _, f0 = _run(model, monkeypatch, False, shape, follow)
    assert took0 == 0 and took1 == int(pruned)
    assert (0 if meta.logits_idx is None else meta.logits_idx.numel()) == rows
    if rows:
        assert h1.shape[0] == rows and S.same_bits(h1, h0)
    assert S.same_bits(kv1, kv0)
    # the step wrote its rows' K / V in every layer: the cache is no longer the filling alone
    fresh = S.new_runner(model).kv
    assert all(not S.same_bits(kv1[l], fresh[l]) for l in range(kv1.shape[0]))
    if follow:
        assert f1.shape[0] == 7 and S.same_bits(f1, f0)


def test_last_layer_cache_write_is_checked(model, monkeypatch):
    """A last block that does not write its K / V: the cache comparison and the follow-up step's
    rows both tell (the test above would catch the omission)."""
    h1, kv1, _, _, f1 = _run(model, monkeypatch, True, S.mixed_333, True)
    real = ops.linear_qkv_fused
    last = model.layers[-1].qkv

    def skip_last(x, w, *a, **k):
        if w is last:
            a = list(a)
            a[7] = a[8] = a[9] = None  # k_cache, v_cache, slots
        return real(x, w, *a, **k)

    monkeypatch.setattr(ops, "linear_qkv_fused", skip_last)
    h2, kv2, _, _, f2 = _run(model, monkeypatch, True, S.mixed_333, True)
    assert S.same_bits(kv1[0], kv2[0]) and not S.same_bits(kv1[1], kv2[1]) and not S.same_bits(f1, f2)


def test_gather_step_reference():
    g = torch.Generator().manual_seed(1)
    T, H, H2, P = 300, 64, 32, 4
    x = torch.randn(T, H, generator=g).to(torch.bfloat16)
    x2 = torch.randn(T, H2, generator=g).to(torch.bfloat16)
    ss = torch.rand(P, T + 20, generator=g)
    pos = torch.randint(0, 1000, (T,), generator=g, dtype=torch.int32)
    for Rn in (1, 129, 256):
        idx = torch.randint(0, T, (Rn,), generator=g)
        idx[-1] = idx[0]  # a repeated row; the order is random, not sorted
        a, b, s, p = ops.gather_step(idx, x, x2, ss, pos, ss_ld=Rn + 3)
        assert torch.equal(a, x[idx]) and torch.equal(b, x2[idx]) and torch.equal(p, pos[idx])
        assert s.shape == (P, Rn + 3) and torch.equal(s[:, :Rn], ss[:, idx])
        a, b, s, p = ops.gather_step(idx, x)
        assert torch.equal(a, x[idx]) and b is None and s is None and p is None
