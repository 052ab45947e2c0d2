"""The last decoder block on the logit rows only (LK_LAST_LAYER_ROWS) against the block on every
row, on the HIP kernels: the same returned hidden rows and the same KV cache in every layer, bit
for bit, for the step shapes of tests/last_layer_steps.py; the gather kernel alone; the row-tile
independence of the one-wave GEMM the identity rests on; and six requests through the engine."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import last_layer_steps as S  # noqa: E402

from llm_kubernetes_minikube_sharp4dev_amd import ops  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.engine.llm_engine import LLMEngine  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.engine.sampling import SamplingParams  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.models import llama as llama_mod  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def model():
    return S.build_model(DEV, BF)


@pytest.fixture(autouse=True)
def _dispatch(monkeypatch):
    # the toy projections have under 16 tiles, which the default dispatch would split over K: a
    # split QKV GEMM has no in-kernel epilogue, so the chain would not be taken at all.  Unsplit,
    # O / gate_up / down of these steps run on the one-wave GEMM's 192-row tiles.
    monkeypatch.setattr(ops, "GEMM_SPLITK", False)
    monkeypatch.setenv("LK_DECODE_TUNE", "0")


def _run(model, monkeypatch, on, shape, follow=False):
    monkeypatch.setattr(llama_mod, "LAST_LAYER_ROWS", on)
    runner = S.new_runner(model)
    items = shape(S.StepMaker())
    si, _ = runner.prepare(items)
    ids, meta = runner._meta(si)
    chain = []
    real = model._forward_chain
    monkeypatch.setattr(model, "_forward_chain", lambda *a, **k: chain.append(1) or real(*a, **k))
    before = model.last_layer_rows
    with torch.inference_mode():
        h = model(ids, meta, runner.kv_caches)
        assert chain == [1], "the fused chain was not taken"
        took = model.last_layer_rows - before
        h2 = None
        if follow:
            si2, _ = runner.prepare(S.follow_up(items))
            ids2, meta2 = runner._meta(si2)
            h2 = model(ids2, meta2, runner.kv_caches).cpu()
    monkeypatch.setattr(model, "_forward_chain", real)
    return h.cpu(), runner.kv.cpu(), took, meta, h2


@pytest.mark.parametrize("shape,rows,pruned", [(S.mixed_333, 6, True), (S.two_tiles, 131, True),
                                               (S.no_logit_rows, 0, False), (S.many_logit_rows, 200, False)])
def test_switch_on_equals_switch_off(model, monkeypatch, shape, rows, pruned):
    """(a) the returned hidden rows and (b) the whole cache of every layer, bit for bit; the mixed
    step is followed by a step that reads the last layer's K / V of every sequence.  ``pruned``:
    whether the gathered-rows branch ran (a counter on the model) -- not with no logit rows, and
    not where they are half of the step's rows."""
    follow = shape is S.mixed_333
    h1, kv1, took1, meta, f1 = _run(model, monkeypatch, True, shape, follow)
    h0, kv0, took0, _, f0 = _run(model, monkeypatch, False, shape, follow)
    assert took0 == 0 and took1 == int(pruned)
    assert (0 if meta.logits_idx is None else meta.logits_idx.numel()) == rows
    if rows:
        assert h1.shape == (rows, 1024) and bool(torch.isfinite(h1.float()).all())
        assert S.same_bits(h1, h0)
    assert S.same_bits(kv1, kv0)
    fresh = S.new_runner(model).kv.cpu()
    assert all(not S.same_bits(kv1[l], fresh[l]) for l in range(kv1.shape[0]))
    if follow:
        assert f1.shape[0] == 7 and S.same_bits(f1, f0)


def test_row_tiles_agree():
    """A row's result on the one-wave GEMM does not depend on the row tile (256 / 192 / 128) nor
    on the rows around it: the RESID and the scaled SwiGLU epilogues on 300 rows, and on 131 of
    those rows gathered, give the same bits -- residual rows, sum-of-squares planes, activations."""
    g = torch.Generator().manual_seed(4)
    M, H, I = 300, 1024, 2048
    x = torch.randn(M, H, generator=g).to(BF).to(DEV)
    w_o = (torch.randn(H, H, generator=g) * 0.03).to(BF).to(DEV)
    w_gu = (torch.randn(2 * I, H, generator=g) * 0.03).to(BF).to(DEV)
    r0 = torch.randn(M, H, generator=g).to(BF).to(DEV)
    idx = torch.randperm(M, generator=g)[:131].to(DEV)
    outs = []
    for v in (3, 4, 5):
        for rows in (None, idx):
            xs, r = (x, r0.clone()) if rows is None else (x[rows].contiguous(), r0[rows].contiguous())
            ss = torch.full((H // 256, xs.shape[0]), -1.0, device=DEV)
            ops.linear_resid(xs, w_o, r, ss, cfg=(v, 256, 1))
            a = ops.linear_swiglu_scaled(r, w_gu, ss, 1e-5, cfg=(v, 256, 1))
            if rows is None:
                r, ss, a = r[idx], ss[:, idx], a[idx]
            outs.append((r.cpu(), ss.cpu().contiguous(), a.cpu()))
    for o in outs[1:]:
        assert all(S.same_bits(p, q) for p, q in zip(o, outs[0]))
    assert bool((outs[0][1] > 0).all()) and bool(outs[0][2].float().abs().sum() > 0)


@pytest.mark.parametrize("R", [1, 129, 256])
def test_gather_step_kernel(R):
    """Residual rows, attention rows, planes and positions of R rows -- repeated and unsorted
    indices -- in one launch; the planes into a sentinel-filled buffer whose columns past R stay."""
    g = torch.Generator().manual_seed(R)
    T, H, H2, P = 333, 1024, 1024 + 8, 4
    x = torch.randn(T, H, generator=g).to(BF).to(DEV)
    x2 = torch.randn(T, 2 * H2, generator=g).to(BF).to(DEV)[:, :H2]  # a strided view
    ss = torch.rand(P, T + 5, generator=g).to(DEV)
    pos = torch.randint(0, 1000, (T,), generator=g, dtype=torch.int32).to(DEV)
    idx = torch.randint(0, T, (R,), generator=g)
    idx[-1] = idx[0]
    idx[R // 2] = T - 1
    idx = idx.to(DEV)
    buf = torch.full((P, R + 7), -7.0, device=DEV)
    a, b, s, p = ops.gather_step(idx, x, x2, ss, pos, ss_out=buf)
    assert s.data_ptr() == buf.data_ptr()
    assert torch.equal(a, x[idx]) and torch.equal(b, x2[idx]) and torch.equal(p, pos[idx])
    assert torch.equal(buf[:, :R], ss[:, idx]) and bool((buf[:, R:] == -7.0).all())
    a, b, s, p = ops.gather_step(idx, x, x2)
    assert torch.equal(a, x[idx]) and torch.equal(b, x2[idx]) and s is None and p is None
    a, b, s, p = ops.gather_step(idx, x, None, ss, None, ss_ld=R + 3)
    assert torch.equal(a, x[idx]) and b is None and p is None and s.shape == (P, R + 3)
    assert torch.equal(s[:, :R], ss[:, idx])


def test_gather_step_refusals():
    x = torch.zeros(8, 64, dtype=BF, device=DEV)
    idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError):  # planes narrower than the step
        ops.gather_step(idx, x, None, torch.zeros(1, 4, device=DEV))
    with pytest.raises(RuntimeError):  # a second source with fewer rows
        ops.gather_step(idx, x, torch.zeros(4, 64, dtype=BF, device=DEV))
    with pytest.raises(RuntimeError):  # a planes buffer narrower than the row list
        ops.gather_step(idx, x, None, torch.zeros(1, 8, device=DEV), ss_out=torch.zeros(1, 1, device=DEV))


def test_engine_same_tokens(model, monkeypatch):
    """Six requests through LLMEngine -- chunked prefill (512-token steps), prefix-cache hits on a
    shared 64-token head, grammar jump-forward -- with the switch on and off: the same token ids."""
    from llm_kubernetes_minikube_sharp4dev_amd.engine import llm_engine

    monkeypatch.setattr(llm_engine, "JUMP_FORWARD", True)
    head = list(range(40, 104))
    prompts = [head + [(7 * i + 3 * j) % 500 + 3 for j in range(90 + 37 * i)] for i in range(6)]

    def proc(hist):  # literal runs between free choices, like the tool-call grammar
        n = len(hist)
        return [(n * 37 + 11) % 512] if n % 7 in (2, 3, 4) else list(range(1 + (n % 5), 512, 3))

    def run(on):
        monkeypatch.setattr(llama_mod, "LAST_LAYER_ROWS", on)
        before = model.last_layer_rows
        eng = LLMEngine(model, None, block_size=16, max_model_len=512, max_num_seqs=8, num_blocks=512,
                        max_num_batched_tokens=512, eos_ids=set(), use_graphs=False)
        eng.generate([prompts[0][:80]], SamplingParams.greedy(2))  # publish the shared head's blocks
        seqs = [eng.add_request(p, SamplingParams.greedy(12, logits_processor=proc)) for p in prompts]
        while eng.has_work():
            eng.step_pipelined()
        eng.flush()
        assert all(len(s.output_ids) == 12 for s in seqs) and eng.steps >= 8
        print(f"switch {on}: {eng.steps} steps, {model.last_layer_rows - before} with a gathered last block")
        assert any(s.num_cached_prefix >= 64 for s in seqs) and any(s.jumped > 0 for s in seqs)
        return [list(s.output_ids) for s in seqs], model.last_layer_rows - before

    on, n_on = run(True)
    off, n_off = run(False)
    assert n_on > 0 and n_off == 0
    assert on == off
