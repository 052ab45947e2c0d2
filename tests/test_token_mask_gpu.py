"""Token masks on the GPU (docs/structured_outputs.md): lk_mask_logits bit for bit against the
fp32 reference on every layout and mask pattern, the sampler's mask rows against the same
allowed sets given as id lists, and schema-constrained requests through the engine."""
import json

import numpy as np
import pytest
import torch

transformers = pytest.importorskip("transformers")

from schema_probes import TOOL, StubTokenizer, validate  # noqa: E402
from test_engine_gpu import PROMPTS, _assert_same_or_near_tie, _gpu_llama  # noqa: E402

from llm_kubernetes_minikube_sharp4dev_amd import ops  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.engine.constrained import json_logits_processor  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.engine.llm_engine import LLMEngine  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.engine.sampling import Sampler, SamplingParams  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.engine.schema_grammar import TokenMask  # noqa: E402
from llm_kubernetes_minikube_sharp4dev_amd.ops import reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG_INF = float("-inf")


def _bits(a: torch.Tensor) -> torch.Tensor:
    return a.contiguous().view(torch.int32 if a.element_size() == 4 else torch.int16).cpu()


def _pool(V: int, seed: int = 0) -> torch.Tensor:
    """int32 [7, words]: 0 random, 1 all ones, 2 all zeros, 3 single bits at 0, 31, 32, V - 1,
    4 alternating bytes, 5 random with every bit beyond V set in the last word, 6 only bits beyond V."""
    words = (V + 31) // 32
    rng = np.random.default_rng(seed)
    p = np.zeros((7, words), dtype=np.uint32)
    p[0] = rng.integers(0, 2**32, words, dtype=np.uint64).astype(np.uint32)
    p[1] = 0xFFFFFFFF
    single = np.zeros(words * 32, dtype=np.uint8)
    single[[i for i in (0, 31, 32, V - 1) if i < V]] = 1
    p[3] = np.packbits(single, bitorder="little").view(np.uint32)
    p[4] = 0xFF00FF00 if V > 8 else 0xAAAAAAAA
    p[5] = rng.integers(0, 2**32, words, dtype=np.uint64).astype(np.uint32)
    beyond = np.zeros(words * 32, dtype=np.uint8)
    beyond[V:] = 1
    p[6] = np.packbits(beyond, bitorder="little").view(np.uint32)
    p[5] |= p[6]
    return torch.from_numpy(p.view(np.int32).copy())


def _logits(B: int, V: int, ls: int, dtype, seed: int = 1) -> torch.Tensor:
    """[B, V] view with row stride ``ls``, NaN (with a payload), +-inf and -0.0 planted in every row."""
    g = torch.Generator().manual_seed(seed)
    full = torch.randn(B, ls, generator=g).to(dtype)
    special = torch.tensor([0x7FC12345 if dtype == torch.float32 else 0x7FC10000, 0x7F800000, -0x00800000, -0x80000000],
                           dtype=torch.int32).view(torch.float32).to(dtype)  # NaN+payload, +inf, -inf, -0.0
    for b in range(B):
        for k in range(4):
            full[b, (b * 5 + k * 2) % V] = special[k]
    return full.to(DEV)[:, :V]


def _check(x, pool, rows, out=None):
    before = _bits(x.clone())
    want = ref.mask_logits(x.cpu(), pool, rows)
    got = ops.mask_logits(x, pool.to(DEV), rows.to(DEV), out=out)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.shape == x.shape
    assert torch.equal(_bits(got), _bits(want))
    if out is None or out.data_ptr() != x.data_ptr():
        assert torch.equal(_bits(x), before)  # the source is never written
    return got


def test_big_vocabulary_bf16():
    V = 128256
    x = _logits(4, V, V, torch.bfloat16)
    assert x.is_contiguous() and x.stride(0) == V
    pool = _pool(V)[[0, 1, 4]]
    got = _check(x, pool, torch.tensor([0, -1, 2, 1], dtype=torch.int32))
    assert torch.equal(_bits(got[1]), _bits(x[1].float())) and torch.equal(_bits(got[3]), _bits(x[3].float()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("V,ls", [(1013, 1013), (1013, 1016), (33, 33), (33, 40), (7, 7), (7, 8), (2048, 2048), (2056, 2056),
                                  (4099, 4104)])
def test_layouts_and_mask_patterns(V, ls, dtype):
    """Odd strides take the element path, aligned ones the 16-byte path with a scalar tail; one
    block and several; every mask pattern, an unconstrained row and a row index outside the pool."""
    pool = _pool(V, seed=V)
    rows = torch.tensor([0, 1, 2, 3, 4, 5, 6, -1, 7, 0], dtype=torch.int32)  # 7 >= R: dead, no fault
    x = _logits(len(rows), V, ls, dtype, seed=ls)
    assert x.stride(0) == ls
    got = _check(x, pool, rows)
    xf = x.float()
    assert torch.equal(_bits(got[1]), _bits(xf[1])) and torch.equal(_bits(got[7]), _bits(xf[7]))  # all ones / no mask: a copy
    assert bool((got[2] == NEG_INF).all()) and bool((got[6] == NEG_INF).all()) and bool((got[8] == NEG_INF).all())
    kept = (got[3].cpu().view(torch.int32) != xf[3].cpu().view(torch.int32)).logical_not().nonzero().flatten().tolist()
    assert set(i for i in (0, 31, 32, V - 1) if i < V) <= set(kept)
    # a padded destination: the columns beyond V keep their sentinel
    for ld in (V + 3, (V + 11) // 4 * 4):
        buf = torch.full((len(rows), ld), 7.25, device=DEV)
        _check(x, pool, rows, out=buf[:, :V])
        assert bool((buf[:, V:] == 7.25).all())


@pytest.mark.parametrize("V,ls", [(1013, 1013), (1016, 1016), (4099, 4100)])
def test_f32_in_place(V, ls):
    pool = _pool(V, seed=3)
    rows = torch.tensor([0, 4, -1, 5, 9], dtype=torch.int32)
    x = _logits(5, V, ls, torch.float32)
    want = ref.mask_logits(x.cpu(), pool, rows)
    pad = _bits(x._base[:, V:]) if x._base is not None and ls > V else None
    got = ops.mask_logits(x, pool.to(DEV), rows.to(DEV), out=x)
    torch.cuda.synchronize()
    assert got.data_ptr() == x.data_ptr() and torch.equal(_bits(x), _bits(want))
    if pad is not None:
        assert torch.equal(_bits(x._base[:, V:]), pad)


def test_edge_cases():
    V = 100
    pool, x = _pool(V).to(DEV), _logits(3, V, 104, torch.bfloat16)
    empty = ops.mask_logits(x[:0], pool, torch.zeros(0, dtype=torch.int32, device=DEV))  # B = 0: nothing launched
    assert empty.shape == (0, V) and empty.dtype == torch.float32
    rows = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
    for bad in (pool[:, :3], torch.cat([pool, pool], dim=1)):  # words != ceil(V / 32)
        with pytest.raises(RuntimeError, match="mask_logits"):
            ops.mask_logits(x, bad.contiguous(), rows)
    # indices at and beyond the pool's end, and INT_MAX: dead rows, the others untouched by them
    rows = torch.tensor([7, 2**31 - 1, 1], dtype=torch.int32, device=DEV)
    got = ops.mask_logits(x, pool, rows)
    torch.cuda.synchronize()
    assert bool((got[:2] == NEG_INF).all()) and torch.equal(_bits(got[2]), _bits(x[2].float()))
    none = ops.mask_logits(x, pool[:0], torch.tensor([0, -1, -5], dtype=torch.int32, device=DEV))  # an empty pool
    assert bool((none[0] == NEG_INF).all()) and torch.equal(_bits(none[1:]), _bits(x[1:].float()))


# ----------------------------------------------------------------------------- sampler
B, V = 6, 4096


@pytest.fixture(scope="module")
def batch():
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(B, V, generator=g) * 3).to(torch.bfloat16).to(DEV)
    rng = np.random.default_rng(2)
    sets = [np.sort(rng.choice(V, size=n, replace=False)) for n in (1, 7, 300, 2048, 4000, 4096)]
    masks = [TokenMask.from_ids(s, V) for s in sets]
    assert all(m.ids().tolist() == s.tolist() for m, s in zip(masks, sets))
    return logits, masks


MODES = {
    "greedy": lambda i, **kw: SamplingParams.greedy(8, **kw),
    "temperature": lambda i, **kw: SamplingParams(temperature=0.8, top_k=0, top_p=1.0, repeat_penalty=1.0, seed=11, **kw),
    "ollama_defaults": lambda i, **kw: SamplingParams(seed=100 + i, **kw),
    "logprobs": lambda i, **kw: SamplingParams(seed=100 + i, logprobs=i in (1, 4), top_logprobs=3 if i == 4 else 0, **kw),
    "greedy_logprobs": lambda i, **kw: SamplingParams.greedy(8, logprobs=i in (0, 3), top_logprobs=2, **kw),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_sampler_mask_rows_equal_list_rows(batch, mode):
    """The same allowed sets as TokenMasks (pool + lk_mask_logits + the batch's selector) and as
    id lists (today's path): the same tokens, step after step, and untouched logits."""
    logits, masks = batch
    mk = MODES[mode]
    lists = [m.ids().tolist() for m in masks]
    pa = [mk(i, logits_processor=lambda h, m=m: m) for i, m in enumerate(masks)]
    pb = [mk(i, logits_processor=lambda h, s=s: s) for i, s in enumerate(lists)]
    sa, sb = Sampler(V, seed=3), Sampler(V, seed=3)
    before = _bits(logits)
    for step in range(3):
        a, b = sa(logits, pa, [[]] * B), sb(logits.clone(), pb, [[]] * B)
        torch.cuda.synchronize()
        assert a.tolist() == b.tolist(), (mode, step)
        assert all(int(t) in m for t, m in zip(a, masks))
        assert torch.equal(_bits(logits), before)  # mask rows never edit the caller's logits
        if "logprobs" in mode:
            assert sa.last_logprobs[:2] == sb.last_logprobs[:2]
            for ta, tb in zip(sa.last_logprobs[2:], sb.last_logprobs[2:]):
                assert torch.equal(ta.cpu(), tb.cpu())
    assert len(sa._mrow_of) == B and getattr(sb, "_mpool", None) is None


@pytest.mark.parametrize("mode", ["greedy", "temperature", "ollama_defaults"])
def test_sampler_mixed_batch(batch, mode):
    """Mask rows, id-list rows and an unconstrained row in one batch: each row its own constraint."""
    logits, masks = batch
    mk = MODES[mode]
    lists = [m.ids().tolist() for m in masks]
    kinds = ["mask", "list", "mask", None, "list", "mask"]
    pa = [mk(i, logits_processor=(None if k is None else (lambda h, m=masks[i]: m) if k == "mask" else
                                  (lambda h, s=lists[i]: s))) for i, k in enumerate(kinds)]
    pb = [mk(i, logits_processor=None if k is None else (lambda h, s=lists[i]: s)) for i, k in enumerate(kinds)]
    sa, sb = Sampler(V, seed=9), Sampler(V, seed=9)
    for step in range(2):
        a, b = sa(logits, pa, [[]] * B), sb(logits.clone(), pb, [[]] * B)
        assert a.tolist() == b.tolist(), (mode, step)
        assert all(k is None or int(t) in masks[i] for i, (t, k) in enumerate(zip(a, kinds)))


# ----------------------------------------------------------------------------- engine
SCHEMA_B = {"type": "object", "properties": {"ok": {"type": "boolean"}, "note": {"type": "string", "maxLength": 6},
                                             "n": {"type": ["integer", "null"]}}, "required": ["ok", "n"]}
SCHEMA_C = {"type": "object", "properties": {"kind": {"const": "pod"},
                                             "tags": {"type": "array", "items": {"enum": ["a", "b", "ab", 10, None]}, "maxItems": 3}},
            "required": ["kind", "tags"]}


def test_engine_schema_requests(monkeypatch):
    """Three concurrent schema requests (greedy, Ollama defaults, greedy with logprobs) under
    pipelined steps with hipGraphs: every output is a complete value of its schema; the greedy
    one is jump-forwarded over its forced runs and equals its step-by-step decoding."""
    from llm_kubernetes_minikube_sharp4dev_amd.engine import llm_engine

    monkeypatch.setenv("LK_DECODE_TUNE", "0")  # both runs on the static GEMM routing, no start-up tuner
    hf, m = _gpu_llama()
    tok = StubTokenizer()

    def run(jf):
        monkeypatch.setattr(llm_engine, "JUMP_FORWARD", jf)
        eng = LLMEngine(m, None, block_size=16, max_model_len=512, max_num_seqs=8, num_blocks=256, eos_ids={511},
                        use_graphs=True)
        sps = [SamplingParams.greedy(160, logits_processor=json_logits_processor(tok, TOOL)),
               SamplingParams(max_tokens=160, seed=4, logits_processor=json_logits_processor(tok, SCHEMA_B)),
               SamplingParams.greedy(160, logits_processor=json_logits_processor(tok, SCHEMA_C), logprobs=True, top_logprobs=2)]
        seqs = [eng.add_request(p, sp) for p, sp in zip(PROMPTS, sps)]
        while eng.has_work():
            eng.step_pipelined()
        eng.flush()
        return seqs

    on = run(True)
    for seq, schema in zip(on, (TOOL, SCHEMA_B, SCHEMA_C)):
        assert seq.finish_reason == "stop" and seq.output_ids[-1] == 511, (seq.finish_reason, tok.decode(seq.output_ids))
        text = tok.decode(seq.output_ids)
        assert validate(json.loads(text), schema) == [], text
    assert on[0].jumped > 0 and on[1].jumped == 0 and on[2].jumped == 0  # the ring / logprobs rows are sampled
    assert len(on[2].logprobs) == len(on[2].output_ids)
    off = run(False)
    assert off[0].jumped == 0 and on[0].steps_run < off[0].steps_run
    _assert_same_or_near_tie(hf, PROMPTS[:1], [on[0].output_ids], [off[0].output_ids])
