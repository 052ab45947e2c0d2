"""Token log-probabilities through the engine on the GPU: six concurrent requests of
different prompt lengths under pipelined stepping, half of them asking.  Every requesting
sequence keeps one entry per output token, the others none; for greedy requests the chosen
token heads its own top list (a wrong row map or logits edited before the kernel read them
would break that); a grammar-constrained request that asks does not jump forward and yields
the text of step-by-step decoding."""
import pytest
import torch

from test_engine_gpu import PROMPTS, _engine, _gpu_llama

from llm_kubernetes_minikube_sharp4dev_amd.engine import llm_engine
from llm_kubernetes_minikube_sharp4dev_amd.engine.sampling import SamplingParams

pytestmark = pytest.mark.gpu
NTOK = 12


@pytest.fixture(scope="module")
def model():
    return _gpu_llama()[1]


@pytest.fixture(autouse=True)
def _static_decode_routing(monkeypatch):
    """Every engine built here skips the start-up decode-GEMM tuner (11 s per engine on an MI355X,
    and not what these tests are about): the static routing table serves the projections."""
    monkeypatch.setenv("LK_DECODE_TUNE", "0")


def _aligned(seq):
    return len(seq.logprobs) == len(seq.output_ids)


@pytest.mark.parametrize("graphs", [False, True])
def test_six_concurrent_requests_pipelined(model, graphs):
    eng = _engine(model, use_graphs=graphs)
    if graphs:
        eng.runner.capture_all(max_batch=8)
    prompts = PROMPTS + [[40, 41, 42, 43, 44, 45, 46]]
    params = [
        SamplingParams.greedy(NTOK, logprobs=True, top_logprobs=0),
        SamplingParams.greedy(NTOK),
        SamplingParams.greedy(NTOK, logprobs=True, top_logprobs=3),
        SamplingParams(temperature=0.8, top_k=40, top_p=0.9, repeat_penalty=1.3, seed=7, max_tokens=NTOK),
        SamplingParams(temperature=0.0, repeat_penalty=1.0, logprobs=True, top_logprobs=20, max_tokens=NTOK),
        SamplingParams(temperature=0.7, top_k=0, top_p=1.0, repeat_penalty=1.0, seed=3, max_tokens=NTOK),
    ]
    want = [p.logprobs for p in params]
    seqs = [eng.add_request(p, sp) for p, sp in zip(prompts[:3], params[:3])]
    it = 0
    while eng.has_work() or len(seqs) < len(prompts):
        if it == 2:  # staggered admission: prefill rows and in-flight decode rows share steps
            seqs += [eng.add_request(p, sp) for p, sp in zip(prompts[3:], params[3:])]
        eng.step_pipelined()
        for s, w in zip(seqs, want):
            assert _aligned(s) if w else s.logprobs == []
        it += 1
    eng.flush()
    assert all(len(s.output_ids) == NTOK for s in seqs)
    for s, sp in zip(seqs, params):
        if not sp.logprobs:
            assert s.logprobs == []
            continue
        assert _aligned(s)
        for tid, (chosen, top) in zip(s.output_ids, s.logprobs):
            assert chosen <= 0.0
            assert len(top) == sp.top_logprobs
            lps = [lp for _, lp in top]
            assert all(a >= b for a, b in zip(lps, lps[1:]))
            if top:  # every requesting request here is greedy without a penalty: its token is the argmax
                assert top[0][0] == tid and top[0][1] == chosen
                assert 0.0 < torch.tensor(lps).exp().sum().item() <= 1.0 + 1e-4  # probabilities of distinct ids
                assert len({i for i, _ in top}) == len(top)


def test_greedy_tokens_unchanged_by_asking(model):
    """The logits path with the kernel attached picks the tokens the logits path alone picks."""
    def run(ask):
        eng = _engine(model, use_graphs=False)
        mk = lambda: SamplingParams.greedy(NTOK, logits_processor=lambda h: None, logprobs=ask, top_logprobs=5 if ask else 0)
        seqs = [eng.add_request(p, mk()) for p in PROMPTS]
        while eng.has_work():
            eng.step_pipelined()
        eng.flush()
        return seqs

    a, b = run(False), run(True)
    assert [s.output_ids for s in a] == [s.output_ids for s in b]
    assert all(_aligned(s) for s in b) and all(s.logprobs == [] for s in a)


def test_grammar_request_does_not_jump(model, monkeypatch):
    def proc(hist):  # literal runs between free choices, like the tool-call grammar
        n = len(hist)
        return [(n * 37 + 11) % 512] if n % 7 in (2, 3, 4) else list(range(1 + (n % 5), 512, 3))

    def run(pipelined, ask):
        eng = _engine(model, use_graphs=False)
        seqs = [eng.add_request(p, SamplingParams.greedy(20, logits_processor=proc, logprobs=ask, top_logprobs=2 if ask else 0))
                for p in PROMPTS[:3]]
        while eng.has_work():
            eng.step_pipelined() if pipelined else eng.step()
        eng.flush()
        return seqs

    asked = run(True, True)
    assert all(s.jumped == 0 and _aligned(s) and len(s.output_ids) == 20 for s in asked)
    monkeypatch.setattr(llm_engine, "JUMP_FORWARD", False)  # the step-by-step run, on a second engine
    plain = run(False, False)
    assert [s.output_ids for s in asked] == [s.output_ids for s in plain]
    # a forced token's logprob is the model's own, not the grammar's: it may be far below 0
    assert all(lp[0] <= 0.0 for s in asked for lp in s.logprobs)
