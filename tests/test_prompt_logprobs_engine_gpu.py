"""Prompt log-probabilities through the engine on the GPU (tiny random-init Llama): a chunked
prompt scores like ONE ``ops.lm_head_logprobs`` call over a single full forward, within the kernel
test's fp32 dot-product bound for this H; no prefix-cache hit; a bystander's tokens do not change."""
import pytest
import torch

from test_engine_gpu import _engine, _gpu_llama
from test_prompt_logprobs_gpu import dot_bound

from llm_kubernetes_minikube_sharp4dev_amd import ops
from llm_kubernetes_minikube_sharp4dev_amd.engine.sampling import SamplingParams

pytestmark = pytest.mark.gpu
PROMPT = [(37 * i + 11) % 500 for i in range(150)]
OTHER = list(range(10, 90))


@pytest.fixture(scope="module")
def model():
    return _gpu_llama()[1]


@pytest.fixture(autouse=True)
def _static_decode_routing(monkeypatch):
    monkeypatch.setenv("LK_DECODE_TUNE", "0")  # no start-up decode-GEMM tuner


def _run(eng, reqs):
    seqs = [eng.add_request(p, sp) for p, sp in reqs]
    while eng.has_work():
        eng.step_pipelined()
    eng.flush()
    return seqs


def test_chunked_prompt_matches_one_full_forward(model):
    eng = _engine(model, use_graphs=False, max_num_batched_tokens=64, token_align=1)
    seq, other = _run(eng, [(PROMPT, SamplingParams.greedy(4, prompt_logprobs=True)), (OTHER, SamplingParams.greedy(6))])
    assert seq.steps_run >= 3 + 3  # the prompt took at least three chunks
    assert len(seq.prompt_logprobs) == len(PROMPT) and seq.prompt_logprobs[0] is None and other.prompt_logprobs == []
    # one forward of the whole prompt, every row kept, one kernel call
    full = _engine(model, use_graphs=False)
    full.add_request(PROMPT, SamplingParams.greedy(1))
    full._drain_inbox()
    si, _ = full.runner.prepare(full.scheduler.schedule().items)
    si.logits_rows = torch.arange(len(PROMPT)).numpy()
    ids, meta = full.runner._meta(si)
    h = model(ids, meta, full.runner.kv_caches)
    tgt = torch.tensor(PROMPT[1:], dtype=torch.int32, device=h.device)
    want = ops.lm_head_logprobs(h[:-1], model.lm_head, tgt, model.vocab_local)[0].cpu().double()
    got = torch.tensor(seq.prompt_logprobs[1:]).double()
    tol = dot_bound(h[:-1].cpu(), model.lm_head.detach().cpu(), model.vocab_local)
    assert (got - want).abs().max() <= tol
    # the same prompt again on the same engine: computed again, not served from the prefix cache
    again, = _run(eng, [(PROMPT, SamplingParams.greedy(1, prompt_logprobs=True))])
    assert again.num_cached_prefix == 0 and again.prompt_logprobs == seq.prompt_logprobs
    # the bystander's tokens are the ones it yields alone
    alone, = _run(_engine(model, use_graphs=False, max_num_batched_tokens=64, token_align=1),
                  [(OTHER, SamplingParams.greedy(6))])
    assert alone.output_ids == other.output_ids
