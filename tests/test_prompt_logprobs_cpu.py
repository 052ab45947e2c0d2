"""Prompt log-probabilities without a GPU (docs/prompt_logprobs.md): reference op, engine, servers."""
import pytest
import torch

from test_logprobs_cpu import MODEL, servers  # noqa: F401  (split-server front end + in-process server)
from test_prompt_logprobs_gpu import exact_inputs, reference

from llm_kubernetes_minikube_sharp4dev_amd import ops
from llm_kubernetes_minikube_sharp4dev_amd.engine.llm_engine import LLMEngine
from llm_kubernetes_minikube_sharp4dev_amd.engine.sampling import SamplingParams
from llm_kubernetes_minikube_sharp4dev_amd.models import build_decoder
from llm_kubernetes_minikube_sharp4dev_amd.serving.engine_core import sp_to_wire


@pytest.mark.parametrize("R,H", [(1, 64), (11, 64), (11, 768)])
def test_reference_op_against_float64(R, H):
    """Exactly summable inputs: only exp / log rounding separates the fp32 op from float64."""
    V = 4 * 128 + 9
    x, w, t = exact_inputs(R, H, V, 128, 3 * 128 + 3)
    want_lp, want_lse = reference(x, w, t, V)
    lp, lse = ops.lm_head_logprobs(x, w, t, V)
    assert lp.dtype == lse.dtype == torch.float32 and lp.shape == lse.shape == (R,)
    assert (lp.double() - want_lp).abs().max() <= 1e-5 and (lse.double() - want_lse).abs().max() <= 1e-5
    t[0] = V  # a padding row's id
    assert ops.lm_head_logprobs(x, w, t, V)[0][0] == float("-inf")


@pytest.fixture(scope="module")
def tiny():
    return build_decoder("llama-tiny", dtype=torch.float32)


def _engine(m, budget):
    return LLMEngine(m, None, max_model_len=512, max_num_seqs=8, num_blocks=128, use_graphs=False, eos_ids=set(),
                     max_num_batched_tokens=budget, token_align=1)


def test_engine_chunked_prefill_matches_the_models_logits(tiny):
    prompt = [(7 * i + 3) % 1000 for i in range(75)]
    eng = _engine(tiny, 32)  # three chunks: boundaries inside the prompt
    seq = eng.add_request(prompt, SamplingParams.greedy(3, prompt_logprobs=True))
    other = eng.add_request(prompt[:20], SamplingParams.greedy(3))
    eng.run_until_done()
    assert seq.steps_run > 3 and other.prompt_logprobs == [] and len(seq.output_ids) == 3
    # one full forward of the same prompt through a fresh cache
    ref_eng = _engine(tiny, 512)
    ref_eng.add_request(prompt, SamplingParams.greedy(1))
    ref_eng._drain_inbox()
    si, _ = ref_eng.runner.prepare(ref_eng.scheduler.schedule().items)
    si.logits_rows = torch.arange(len(prompt)).numpy()
    ids, meta = ref_eng.runner._meta(si)
    lg = tiny.logits(tiny(ids, meta, ref_eng.runner.kv_caches))
    want = torch.log_softmax(lg.double(), -1)[:-1].gather(1, torch.tensor(prompt[1:])[:, None]).squeeze(1)
    assert seq.prompt_logprobs[0] is None and len(seq.prompt_logprobs) == len(prompt)
    assert (torch.tensor(seq.prompt_logprobs[1:]).double() - want).abs().max() < 1e-4
    # the same prompt again: no prefix-cache hit for a requesting request, the same list
    again = eng.add_request(prompt, SamplingParams.greedy(1, prompt_logprobs=True))
    eng.run_until_done()
    assert again.num_cached_prefix == 0 and again.prompt_logprobs == seq.prompt_logprobs


def test_echo_scores_the_prompt_on_both_servers(servers):
    c_fe, c_local = servers
    assert "prompt_logprobs" not in sp_to_wire(SamplingParams())  # the wire field travels only when set
    assert SamplingParams(**sp_to_wire(SamplingParams(prompt_logprobs=True))).prompt_logprobs
    prompt = "kubectl get pods --all-namespaces shows CrashLoopBackOff"
    body = {"model": MODEL, "prompt": prompt, "echo": True, "logprobs": 0, "max_tokens": 0, "temperature": 0}
    a, b = c_local.post("/v1/completions", json=body).json(), c_fe.post("/v1/completions", json=body).json()
    ids = [0] * a["usage"]["prompt_tokens"]
    for r in (a, b):  # b: the list rode on the request's final frame
        ch = r["choices"][0]
        lp = ch["logprobs"]
        assert ch["text"] == prompt and len(ids) > 4
        assert r["usage"] == {"prompt_tokens": len(ids), "completion_tokens": 0, "total_tokens": len(ids)}
        assert len(lp["tokens"]) == len(lp["token_logprobs"]) == len(lp["text_offset"]) == len(ids)
        assert "".join(lp["tokens"][1:]) == prompt and lp["text_offset"][1] == 0
        assert lp["token_logprobs"][0] is None and all(v < 0 for v in lp["token_logprobs"][1:])
        assert lp["top_logprobs"] == [None] * len(ids)
    assert max(abs(x - y) for x, y in zip(a["choices"][0]["logprobs"]["token_logprobs"][1:],
                                          b["choices"][0]["logprobs"]["token_logprobs"][1:])) < 1e-4
    # with a completion: the prompt's entries first, then the generated tokens'
    r = c_local.post("/v1/completions", json=dict(body, max_tokens=3, logprobs=2)).json()
    lp = r["choices"][0]["logprobs"]
    assert r["choices"][0]["text"].startswith(prompt) and r["usage"]["completion_tokens"] == 3
    assert len(lp["tokens"]) == len(ids) + 3 and all(len(t) == 2 for t in lp["top_logprobs"][len(ids):])


def test_echo_validation_and_unchanged_responses(servers):
    c_fe, c_local = servers
    for c in (c_fe, c_local):
        r = c.post("/v1/completions", json={"model": MODEL, "prompt": "ciao", "echo": True, "stream": True})
        assert r.status_code == 400 and "stream" in r.json()["error"]["message"]
        plain = c.post("/v1/completions", json={"model": MODEL, "prompt": "ciao", "max_tokens": 2}).json()
        assert sorted(plain) == ["choices", "created", "id", "model", "object"]
        assert sorted(plain["choices"][0]) == ["finish_reason", "index", "text"]
