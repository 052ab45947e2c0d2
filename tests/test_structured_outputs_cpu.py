"""Structured outputs on the CPU (docs/structured_outputs.md): the mask reference, the schema
grammar's properties over the built-in 32k tokenizer, the per-request cursor, the sampler's mask
pool, and the HTTP routes (in-process and through the split server)."""
import json
import os
import random
import tempfile

import numpy as np
import pytest
import torch
from fastapi.testclient import TestClient

from schema_probes import (ACTIONS, REFUSED, SCHEMAS, TOOL, StubTokenizer, compact, pieces_by_text, random_walk, tokenise,
                           validate)

from llm_kubernetes_minikube_sharp4dev_amd import ops
from llm_kubernetes_minikube_sharp4dev_amd.config import Config
from llm_kubernetes_minikube_sharp4dev_amd.engine import sampling
from llm_kubernetes_minikube_sharp4dev_amd.engine.constrained import JsonGrammar, json_logits_processor
from llm_kubernetes_minikube_sharp4dev_amd.engine.sampling import Sampler, SamplingParams
from llm_kubernetes_minikube_sharp4dev_amd.engine.schema_grammar import (SchemaCursor, SchemaGrammar, TokenMask, compiled)
from llm_kubernetes_minikube_sharp4dev_amd.models.tokenizer import builtin_tokenizer
from llm_kubernetes_minikube_sharp4dev_amd.ops import reference as ref


@pytest.fixture(scope="module")
def tok():
    return builtin_tokenizer()


@pytest.fixture(scope="module")
def by_text(tok):
    return pieces_by_text(tok)


# ----------------------------------------------------------------------------- reference op
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_ref_mask_logits_against_a_loop(dtype):
    g = torch.Generator().manual_seed(3)
    B, V, R = 5, 75, 3
    words = (V + 31) // 32
    x = torch.randn(B, V, generator=g).to(dtype)
    x[0, 3], x[1, 4], x[2, 5], x[3, 6] = float("nan"), float("inf"), float("-inf"), -0.0
    pool = torch.randint(-2**31, 2**31 - 1, (R, words), generator=g, dtype=torch.int64).to(torch.int32)
    rows = torch.tensor([0, -1, 2, 3, 1], dtype=torch.int32)  # 3 >= R: a dead row
    got = ref.mask_logits(x, pool, rows)
    assert got.dtype == torch.float32 and got.shape == (B, V)
    want = torch.empty(B, V, dtype=torch.float32)
    pu = pool.numpy().view(np.uint32)
    for b in range(B):
        for v in range(V):
            r = int(rows[b])
            keep = r < 0 or (r < R and (int(pu[r, v >> 5]) >> (v & 31)) & 1)
            want[b, v] = x[b, v].float() if keep else float("-inf")
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # byte v >> 3 of a row is np.packbits(bits, bitorder="little")[v >> 3]
    bits = np.zeros(words * 32, dtype=np.uint8)
    bits[[0, 9, 31, 32, 74]] = 1
    p1 = torch.from_numpy(np.packbits(bits, bitorder="little").view(np.int32).copy())[None]
    one = ref.mask_logits(x[:1], p1, torch.zeros(1, dtype=torch.int32))
    assert (one[0] != float("-inf")).nonzero().flatten().tolist() == [0, 9, 31, 32, 74]
    with pytest.raises(ValueError):
        ref.mask_logits(x, pool[:, :2], rows)
    out = torch.full((B, V + 5), 7.0)
    ref.mask_logits(x, pool, rows, out=out[:, :V])
    assert torch.equal(out[:, :V].view(torch.int32), want.view(torch.int32)) and bool((out[:, V:] == 7.0).all())
    routed = ops.mask_logits(x, pool, rows)  # CPU tensors route to the reference
    assert torch.equal(routed.view(torch.int32), got.view(torch.int32))
    assert ops.mask_logits(x[:0], pool, rows[:0]).shape == (0, V)


def test_token_mask_is_a_sequence():
    m = TokenMask.from_ids([70, 3, 31, 32, 3], 75)
    assert len(m) == 4 and int(m[0]) == 3 and m.ids().tolist() == [3, 31, 32, 70] and m.ids().dtype == np.int64
    assert m.words.dtype == np.uint32 and m.words.size == 3 and not m.words.flags.writeable
    assert 31 in m and 33 not in m and 10**6 not in m
    assert bytes(m.words.view(np.uint8)) == bytes(np.packbits(np.isin(np.arange(96), [3, 31, 32, 70]), bitorder="little"))


# ----------------------------------------------------------------------------- grammar
@pytest.mark.parametrize("name,schema,instances,must_finish", SCHEMAS, ids=[s[0] for s in SCHEMAS])
def test_random_walks_validate(tok, name, schema, instances, must_finish):
    """A uniformly random allowed token per step: every walk that ends is compact JSON that
    validates against its schema."""
    rng = random.Random(len(name) * 7919 + 1)
    done = 0
    for _ in range(6):
        ids, finished = random_walk(json_logits_processor(tok, schema), tok.eos_ids, rng, 250)
        if not finished:
            assert not must_finish, tok.decode(ids)
            continue
        done += 1
        text = tok.decode(ids)
        v = json.loads(text)
        assert validate(v, schema) == [], (text, validate(v, schema))
        # compact: no whitespace outside strings
        assert not any(c in " \t\n\r" for c in compact(_blank_strings(v))) and _no_outer_ws(text)
    assert done or not must_finish


def _blank_strings(v):
    if isinstance(v, str):
        return ""
    if isinstance(v, list):
        return [_blank_strings(x) for x in v]
    if isinstance(v, dict):
        return {"": _blank_strings(x) for x in v.values()} if v else {}
    return v


def _no_outer_ws(text: str) -> bool:
    in_str, esc = False, False
    for c in text:
        if in_str:
            if esc:
                esc = False
            elif c == "\\":
                esc = True
            elif c == '"':
                in_str = False
        elif c == '"':
            in_str = True
        elif c in " \t\n\r":
            return False
    return True


RAW = {"numbers": ["[-1.5,2e10,3.25E-3]", "[0]", "[-0.0e+12]"], "nullable": ['"\\u00e9\\n"'], "enum_mixed": ["123"]}


@pytest.mark.parametrize("name,schema,instances,must_finish", SCHEMAS, ids=[s[0] for s in SCHEMAS])
def test_every_prefix_of_a_valid_text_is_accepted(tok, by_text, name, schema, instances, must_finish):
    for text in [compact(v) for v in instances] + RAW.get(name, []):
        assert validate(json.loads(text), schema) == []  # the instance itself
        proc = json_logits_processor(tok, schema)
        ids, _ = tokenise(proc, tok, text, by_text)
        assert tok.decode(ids) == text
        end = proc(ids)
        assert all(e in end for e in tok.eos_ids), text  # complete: the request may end here
        g = proc.grammar
        if not g.final(g.feed_text(g.start, text)) or g.feed_text(g.start, text) == ():
            assert sorted(end.ids().tolist()) == sorted(tok.eos_ids)  # closed: nothing but the end


def test_invalid_texts_are_rejected(tok):
    bad = [(TOOL, '{"action":"gex'), (TOOL, '{"r'), (TOOL, '{"action":"get_logs"}'), (TOOL, '{ '),
           (TOOL, '{"action":"get_logs","replicas":1.'), (TOOL, '{"action":"get_logs","replicas":01'),
           (TOOL, '{"action":"get_logs","replicas":1,'), ({"type": "string", "maxLength": 2}, '"abc'),
           ({"type": "string", "minLength": 2}, '"a"'), ({"type": "string"}, '"\t'), ({"type": "string"}, '"\\x'),
           ({"type": "array", "items": {"type": "integer"}, "maxItems": 1}, "[1,"), ({"type": "array", "minItems": 1}, "[]"),
           ({"type": "integer"}, "1e"), ({"type": "number"}, "1.e"), ({"type": "boolean"}, "trx"), ({}, "[1, "),
           ({"type": "object"}, "[")]
    for schema, text in bad:
        g = SchemaGrammar(tok, schema)
        assert g.feed_text(g.start, text[:-1]) is not None, (schema, text)
        assert g.feed_text(g.start, text) is None, (schema, text)
    deep = SchemaGrammar(tok, {})
    assert deep.feed_text(deep.start, "[" * 16) is not None and deep.feed_text(deep.start, "[" * 17) is None


@pytest.mark.parametrize("keyword,schema", REFUSED, ids=[f"{k}-{i}" for i, (k, _) in enumerate(REFUSED)])
def test_unsupported_schemas_raise_naming_the_keyword(tok, keyword, schema):
    with pytest.raises(ValueError, match=keyword.replace("$", r"\$")):
        json_logits_processor(tok, schema)


def test_nesting_bound(tok):
    s = {"type": "integer"}
    for _ in range(16):
        s = {"type": "array", "items": s}
    json_logits_processor(tok, s)
    with pytest.raises(ValueError, match="16"):
        json_logits_processor(tok, {"type": "array", "items": s})


def test_format_json_and_none_keep_the_json_grammar(tok):
    assert type(json_logits_processor(tok)) is JsonGrammar and type(json_logits_processor(tok, None)) is JsonGrammar
    assert isinstance(json_logits_processor(tok, TOOL), SchemaCursor)


def test_forced_runs_give_one_bit_masks():
    """Keys, punctuation, a const and the rest of an enum value once its prefix is unique: one
    allowed token, the longest piece spelling a prefix of the run."""
    st = StubTokenizer()
    g = SchemaGrammar(st, TOOL)
    assert g.forced_run(g.start) == '{"action":"'
    cur = g.cursor()
    ids = []
    m = cur(ids)
    assert len(m) == 1 and st.piece(int(m[0])) == '{"action":"'  # the longest piece, not '{' or '{"'
    ids.append(int(m[0]))
    m = cur(ids)  # the enum: l / g / s / c / f and the pieces that start a value
    assert {st.piece(int(i)) for i in m.ids()} == {"l", "g", "s", "c", "f", "list", "get", "scale", "cluster", "final"}
    ids.append(st.pieces.index("s"))
    run = []
    while True:
        m = cur(ids)
        if len(m) != 1:
            break
        run.append(st.piece(int(m[0])))
        ids.append(int(m[0]))
    assert "".join(run) == 'cale_deployment","replicas":' and run[0] == "c" and '","' in run and "replicas" in run
    assert all(st.piece(int(i))[0] in "-0123456789" for i in m.ids()) and len(m) > 10
    ids.append(st.pieces.index("12"))
    assert {st.piece(int(i)) for i in cur(ids).ids()} == set("0123456789}") | {"10", "12", "100"}
    ids.append(st.pieces.index("}"))
    assert cur(ids).ids().tolist() == [511]
    # a const object is one forced run from the first token to the last
    gc = SchemaGrammar(st, {"type": "object", "properties": {"k": {"const": "v"}, "n": {"const": None}}, "required": ["k", "n"]})
    cur, ids = gc.cursor(), []
    while st.decode(ids) != '{"k":"v","n":null}':
        m = cur(ids)
        assert len(m) == 1
        ids.append(int(m[0]))
    assert len(ids) < len('{"k":"v","n":null}') and cur(ids).ids().tolist() == [511]
    # without end-of-sequence ids the closed state allows id 0, as JsonGrammar does
    st2 = StubTokenizer()
    st2.eos_ids = set()
    st2.pieces[511] = "�"
    g2 = SchemaGrammar(st2, {"const": 1})
    assert g2.mask(()).ids().tolist() == [0]


def test_masks_are_cached_per_state_and_counted_strings_collapse(tok):
    g = SchemaGrammar(tok, {"type": "string", "maxLength": 200})
    far = [g.mask(g.feed_text(g.start, '"' + "a" * n)) for n in (0, 1, 50, 100)]
    assert all(m is far[0] for m in far) and g.mask_builds == 1  # further from the limit than the longest piece
    near = g.mask(g.feed_text(g.start, '"' + "a" * 198))
    assert near is not far[0] and len(near) < len(far[0])  # 2 characters of room left
    assert all(len(p) <= 2 or '"' in p or "\\" in p for p in (tok.piece(int(i)) for i in near.ids()))
    # compiled grammars are shared per (tokenizer, schema text): two requests get the same mask objects
    a, b = json_logits_processor(tok, TOOL), json_logits_processor(tok, json.loads(json.dumps(TOOL)))
    assert a is not b and a.grammar is b.grammar is compiled(tok, TOOL) and a([]) is b([])
    # declaration order is the emission order: it is part of the key
    swapped = dict(TOOL, properties=dict(reversed(list(TOOL["properties"].items()))))
    assert compiled(tok, swapped) is not a.grammar


def test_cursor_same_ids_jump_and_divergence(tok, by_text):
    text = compact({"action": "scale_deployment", "replicas": 12})
    ids, forced = tokenise(json_logits_processor(tok, TOOL), tok, text, by_text)
    assert forced > 3
    g = compiled(tok, TOOL)
    fresh = lambda upto: g.mask(g.feed_text(g.start, tok.decode(ids[:upto])))  # noqa: E731
    cur = g.cursor()
    assert cur(ids[:2]) is fresh(2) and cur(ids[:2]) is fresh(2)        # the same ids again
    assert cur(ids[:7]) is fresh(7) and len(cur._ids) == 7                # several ids longer (after a jump)
    assert cur(ids[:3]) is fresh(3) and len(cur._ids) == 3                # shorter: back to the cached prefix
    other = ids[:4] + [by_text["x"]] + ids[5:6]
    assert cur(other).ids().tolist() == sorted(tok.eos_ids)                # left the grammar: only the end
    assert cur(ids) is fresh(len(ids)) and cur(ids + [next(iter(tok.eos_ids))]) is fresh(len(ids))
    hist = []  # the engine's usage: one list object that grows
    cur2 = g.cursor()
    for t in ids:
        assert t in cur2(hist)
        hist.append(t)
    assert sorted(cur2(hist).ids().tolist()) == sorted(tok.eos_ids) and len(cur2._states) == len(ids) + 1


# ----------------------------------------------------------------------------- sampler pool
def _mask_procs(V, sets):
    masks = [TokenMask.from_ids(s, V) for s in sets]
    return masks, [lambda h, m=m: m for m in masks]


def test_sampler_mask_rows_equal_list_rows_cpu():
    V, B = 300, 5
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(B, V, generator=g)
    sets = [sorted(random.Random(i).sample(range(V), 1 + 40 * i)) for i in range(B)]
    masks, procs = _mask_procs(V, sets)
    for mk in (lambda **kw: SamplingParams.greedy(4, **kw), lambda **kw: SamplingParams(seed=5, **kw)):
        a = Sampler(V, seed=1)(logits.clone(), [mk(logits_processor=p) for p in procs], [[]] * B)
        b = Sampler(V, seed=1)(logits.clone(), [mk(logits_processor=lambda h, s=s: s) for s in sets], [[]] * B)
        assert a.tolist() == b.tolist() and all(int(t) in s for t, s in zip(a, sets))
    # mixed: mask row, list row, unconstrained row, and logprobs leave the logits alone
    keep = logits.clone()
    s = Sampler(V, seed=1)
    ps = [SamplingParams.greedy(4, logits_processor=procs[0]), SamplingParams.greedy(4, logits_processor=lambda h: sets[1]),
          SamplingParams.greedy(4, logprobs=True, top_logprobs=2), SamplingParams.greedy(4, logits_processor=procs[3], logprobs=True)]
    out = s(logits[:4], ps, [[]] * 4)
    assert torch.equal(logits, keep) and s.last_logprobs[0] == [2, 3]
    for i, allowed in enumerate([sets[0], sets[1], range(V), sets[3]]):
        assert int(out[i]) == max(allowed, key=lambda t: (float(logits[i, t]), -t))


def test_pool_lru_eviction_live_rows_and_padding():
    V = 70
    s = Sampler(V)
    s.MASK_ROWS = 4
    logits = torch.zeros(3, V)
    mk = lambda m: SamplingParams.greedy(1, logits_processor=lambda h: m)  # noqa: E731
    masks = [TokenMask.from_ids([i, i + 1], V) for i in range(8)]
    assert getattr(s, "_mpool", None) is None
    s(logits, [mk(masks[0]), mk(masks[1]), mk(masks[0])], [[]] * 3)
    assert s._mpool.shape == (4, 3) and s._mpool.dtype == torch.int32 and len(s._mrow_of) == 2
    r0, r1 = s._mrow_of[id(masks[0])][1], s._mrow_of[id(masks[1])][1]
    s(logits[:2], [mk(masks[2]), mk(masks[3])], [[]] * 2)
    assert len(s._mrow_of) == 4 and not s._mfree
    s(logits[:1], [mk(masks[0])], [[]])            # touch 0: 1 is now the least recently used
    out = s(logits[:2], [mk(masks[4]), mk(masks[0])], [[]] * 2)
    assert id(masks[1]) not in s._mrow_of and s._mrow_of[id(masks[4])][1] == r1 and s._mrow_of[id(masks[0])][1] == r0
    assert out.tolist() == [4, 0]
    # a batch never evicts its own rows: 4 masks in a 4-row pool, all new but one
    out = s(logits.repeat(2, 1)[:4], [mk(masks[5]), mk(masks[6]), mk(masks[7]), mk(masks[0])], [[]] * 4)
    assert out.tolist() == [5, 6, 7, 0] and set(s._mrow_of) == {id(masks[i]) for i in (5, 6, 7, 0)}
    assert sorted(e[1] for e in s._mrow_of.values()) == [0, 1, 2, 3]
    for m in (masks[5], masks[0]):  # the pool row holds the mask's words
        assert s._mpool[s._mrow_of[id(m)][1]].numpy().view(np.uint32).tolist() == m.words.tolist()
    with pytest.raises(RuntimeError, match="distinct token masks"):
        s(torch.zeros(5, V), [mk(m) for m in masks[:5]], [[]] * 5)
    # tokenizer vocabulary smaller / larger than the logits' V: padded with zeros / truncated
    small, big = TokenMask.from_ids([1, 40], 41), TokenMask.from_ids([2, 69, 100, 200], 256)
    lg = torch.zeros(2, V)
    lg[:, 69] = 1.0
    out = Sampler(V)(lg, [mk(small), mk(big)], [[]] * 2)
    assert out.tolist() == [1, 69]
    lg[1, 69] = float("-inf")
    assert Sampler(V)(lg, [mk(small), mk(big)], [[]] * 2).tolist() == [1, 2]  # ids >= V are not there


def test_batches_without_schema_rows_never_reach_the_mask_kernel(monkeypatch):
    calls = []
    real = ops.mask_logits
    monkeypatch.setattr(ops, "mask_logits", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    assert sampling.ops is ops
    V = 64
    logits = torch.randn(3, V, generator=torch.Generator().manual_seed(1))
    s = Sampler(V)
    lists = [SamplingParams.greedy(1, logits_processor=lambda h: [1, 2, 3]), SamplingParams(seed=1),
             SamplingParams(seed=2, logits_processor=lambda h: None, logprobs=True)]
    s(logits.clone(), lists, [[]] * 3)
    s(logits.clone(), [SamplingParams.greedy(1)] * 3, [[]] * 3)
    assert calls == [] and getattr(s, "_mpool", None) is None
    m = TokenMask.from_ids([5, 6], V)
    s(logits.clone(), lists[:2] + [SamplingParams.greedy(1, logits_processor=lambda h: m)], [[]] * 3)
    assert calls == [1]


# ----------------------------------------------------------------------------- HTTP
ALIASES = {"llama3.1:8b": "llama-tiny", "nomic-embed-text": "bert-tiny"}
MODEL = "llama3.1:8b"


def _cfg():
    cfg = Config()
    cfg.engine.max_model_len = 2048
    cfg.engine.default_max_new_tokens = 8
    return cfg


@pytest.fixture(scope="module")
def server():
    from llm_kubernetes_minikube_sharp4dev_amd.serving.model_manager import ModelManager
    from llm_kubernetes_minikube_sharp4dev_amd.serving.ollama_server import create_app

    mgr = ModelManager(_cfg(), device="cpu", aliases=ALIASES)
    with TestClient(create_app(mgr)) as c:
        yield c
    mgr.shutdown()


def _check_tool(text):
    v = json.loads(text)
    assert validate(v, TOOL) == [] and text == compact(v), text
    assert list(v) == ["action", "replicas"] and v["action"] in ACTIONS
    return v


def test_api_generate_enforces_the_schema(server):
    """(fails where the schema of ``format`` is ignored: the tiny model's free JSON is no tool call)"""
    for opts in ({"num_predict": 64, "temperature": 0}, {"num_predict": 64, "seed": 3}):
        r = server.post("/api/generate", json={"model": MODEL, "prompt": "scale it", "stream": False, "format": TOOL,
                                               "options": opts})
        assert r.status_code == 200, r.text
        assert r.json()["done_reason"] == "stop"
        _check_tool(r.json()["response"])


def test_api_chat_and_openai_enforce_the_schema(server):
    msgs = [{"role": "user", "content": "scale it"}]
    r = server.post("/api/chat", json={"model": MODEL, "messages": msgs, "stream": False, "format": TOOL,
                                       "options": {"num_predict": 64, "temperature": 0}})
    assert r.status_code == 200, r.text
    _check_tool(r.json()["message"]["content"])
    body = {"model": MODEL, "messages": msgs, "max_tokens": 64, "temperature": 0}
    rf = {"type": "json_schema", "json_schema": {"name": "tool", "schema": TOOL}}
    r = server.post("/v1/chat/completions", json={**body, "response_format": rf})
    assert r.status_code == 200, r.text
    _check_tool(r.json()["choices"][0]["message"]["content"])
    assert r.json()["choices"][0]["finish_reason"] == "stop"
    r = server.post("/v1/chat/completions", json={**body, "max_tokens": 24, "response_format": {"type": "json_object"}})
    from llm_kubernetes_minikube_sharp4dev_amd.engine.constrained import JSON_START, json_feed_text

    assert r.status_code == 200 and json_feed_text(JSON_START, r.json()["choices"][0]["message"]["content"]) is not None
    free = server.post("/v1/chat/completions", json={**body, "max_tokens": 6}).json()
    text = server.post("/v1/chat/completions", json={**body, "max_tokens": 6, "response_format": {"type": "text"}}).json()
    assert free["choices"][0]["message"] == text["choices"][0]["message"]


def test_bad_schemas_and_response_formats_are_400s(server):
    msgs = [{"role": "user", "content": "x"}]
    bad = {"type": "object", "properties": {"when": {"type": "string", "format": "date-time"}}}
    for route, body in (("/api/generate", {"model": MODEL, "prompt": "x", "stream": False, "format": bad}),
                        ("/api/chat", {"model": MODEL, "messages": msgs, "stream": False, "format": bad})):
        r = server.post(route, json=body)
        assert r.status_code == 400 and "'format'" in r.json()["error"], r.text
    r = server.post("/api/generate", json={"model": MODEL, "prompt": "x", "stream": False,
                                           "format": {"type": "integer", "minimum": 3}})
    assert r.status_code == 400 and "minimum" in r.json()["error"]
    oa = {"model": MODEL, "messages": msgs, "max_tokens": 4}
    for rf, word in (({"type": "json_schema", "json_schema": {"schema": bad}}, "'format'"),
                     ({"type": "json_schema", "json_schema": {"schema": {"not": {}}}}, "'not'"),
                     ({"type": "json_schema"}, "response_format.json_schema.schema"),
                     ({"type": "json_schema", "json_schema": {"schema": [1]}}, "response_format.json_schema.schema"),
                     ({"type": "yaml"}, "response_format.type"), ("json", "response_format.type"),
                     ({}, "response_format.type")):
        r = server.post("/v1/chat/completions", json={**oa, "response_format": rf})
        assert r.status_code == 400, (rf, r.text)
        err = r.json()["error"]
        assert err["type"] == "invalid_request_error" and word in err["message"], (rf, err)


def test_split_server_gives_the_same_text(server):
    from llm_kubernetes_minikube_sharp4dev_amd.serving.engine_core import EngineCore
    from llm_kubernetes_minikube_sharp4dev_amd.serving.model_manager import ModelManager
    from llm_kubernetes_minikube_sharp4dev_amd.serving.remote import create_frontend_app

    mgr = ModelManager(_cfg(), device="cpu", aliases=ALIASES)
    core = EngineCore(mgr, os.path.join(tempfile.mkdtemp(), "core0.sock"))
    try:
        fe = create_frontend_app([core.path], _cfg(), ALIASES, preload=[MODEL])
        with TestClient(fe) as c_fe:
            body = {"model": MODEL, "prompt": "scale it", "stream": False, "format": TOOL,
                    "options": {"num_predict": 64, "temperature": 0}}
            a, b = c_fe.post("/api/generate", json=body), server.post("/api/generate", json=body)
            assert a.status_code == b.status_code == 200, (a.text, b.text)
            assert a.json()["response"] == b.json()["response"]
            _check_tool(a.json()["response"])
            oa = {"model": MODEL, "messages": [{"role": "user", "content": "scale it"}], "max_tokens": 64, "temperature": 0,
                  "response_format": {"type": "json_schema", "json_schema": {"schema": TOOL}}}
            a, b = c_fe.post("/v1/chat/completions", json=oa), server.post("/v1/chat/completions", json=oa)
            assert a.json()["choices"][0]["message"] == b.json()["choices"][0]["message"]
            _check_tool(a.json()["choices"][0]["message"]["content"])
            # refused by the front-end: nothing reaches the core
            served = core_served(fe)
            r = c_fe.post("/api/generate", json={**body, "format": {"type": "string", "pattern": "a+"}})
            assert r.status_code == 400 and "pattern" in r.json()["error"] and core_served(fe) == served
    finally:
        core.close()
        mgr.shutdown()


def core_served(fe) -> int:
    pool = getattr(fe.state, "pool", None)
    return sum(c.served for c in pool.cores) if pool is not None and hasattr(pool, "cores") else -1
