"""Shared pieces of the structured-output tests: a small JSON-schema validator for the
supported subset (written against the JSON Schema specification, independently of the grammar
code: it checks parsed values, the grammar generates text), the schemas with one valid instance
each, a 512-piece stub tokenizer, and the walk / tokenise helpers."""
import json
import random

# ----------------------------------------------------------------------------- validator
_ANNOT = {"title", "description", "default", "examples", "$schema", "$id", "$defs", "definitions"}


def _type_ok(v, t):
    if t == "null":
        return v is None
    if t == "boolean":
        return isinstance(v, bool)
    if t == "string":
        return isinstance(v, str)
    if t == "array":
        return isinstance(v, list)
    if t == "object":
        return isinstance(v, dict)
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        return False
    return True if t == "number" else (isinstance(v, int) or v == int(v))


def _equal(a, b):
    if isinstance(a, bool) or isinstance(b, bool) or a is None or b is None:
        return type(a) is type(b) and a == b
    return a == b


def validate(v, schema, root=None):
    """[] if ``v`` conforms to ``schema``, else a list of reasons."""
    root = schema if root is None else root
    if schema is True or schema == {}:
        return []
    errs = []
    if "$ref" in schema:
        _, group, name = schema["$ref"].split("/", 2)
        return validate(v, root[group][name], root)
    if "type" in schema:
        ts = schema["type"] if isinstance(schema["type"], list) else [schema["type"]]
        if not any(_type_ok(v, t) for t in ts):
            errs.append(f"{v!r} is not of type {ts}")
    if "enum" in schema and not any(_equal(v, e) for e in schema["enum"]):
        errs.append(f"{v!r} not in enum {schema['enum']}")
    if "const" in schema and not _equal(v, schema["const"]):
        errs.append(f"{v!r} is not {schema['const']!r}")
    if isinstance(v, str):
        if len(v) < schema.get("minLength", 0):
            errs.append(f"{v!r} shorter than {schema['minLength']}")
        if "maxLength" in schema and len(v) > schema["maxLength"]:
            errs.append(f"{v!r} longer than {schema['maxLength']}")
    if isinstance(v, list):
        if len(v) < schema.get("minItems", 0):
            errs.append(f"{len(v)} items, fewer than {schema['minItems']}")
        if "maxItems" in schema and len(v) > schema["maxItems"]:
            errs.append(f"{len(v)} items, more than {schema['maxItems']}")
        if "items" in schema:
            for x in v:
                errs += validate(x, schema["items"], root)
    if isinstance(v, dict):
        props = schema.get("properties", {})
        for r in schema.get("required", []):
            if r not in v:
                errs.append(f"required {r!r} missing")
        for k, x in v.items():
            if k in props:
                errs += validate(x, props[k], root)
            elif schema.get("additionalProperties") is False:
                errs.append(f"additional property {k!r}")
            elif isinstance(schema.get("additionalProperties"), dict):
                errs += validate(x, schema["additionalProperties"], root)
    if "anyOf" in schema and not any(not validate(v, a, root) for a in schema["anyOf"]):
        errs.append(f"{v!r} matches no anyOf alternative")
    if "oneOf" in schema and sum(1 for a in schema["oneOf"] if not validate(v, a, root)) != 1:
        errs.append(f"{v!r} does not match exactly one oneOf alternative")
    return errs


# ----------------------------------------------------------------------------- schemas
ACTIONS = ["list_pods", "get_logs", "scale_deployment", "cluster_context", "final_answer"]
TOOL = {"type": "object", "properties": {"action": {"enum": ACTIONS}, "replicas": {"type": "integer"}},
        "required": ["action", "replicas"], "additionalProperties": False}

# (name, schema, valid instances, every walk must finish)
SCHEMAS = [
    ("tool", TOOL, [{"action": "get_logs", "replicas": 3}, {"action": "final_answer", "replicas": -120}], True),
    ("optional", {"type": "object", "title": "t", "description": "d",
                  "properties": {"a": {"type": "boolean"}, "b": {"type": "null"}, "c": {"type": "string", "maxLength": 6},
                                 "d": {"type": "integer", "default": 1}},
                  "required": ["b"]},
     [{"b": None}, {"a": True, "b": None, "d": 0}, {"b": None, "c": "x\"y\\n", "d": 12}, {"a": False, "b": None, "c": ""}], True),
    ("strings", {"type": "object", "properties": {"s": {"type": "string", "minLength": 2, "maxLength": 5},
                                                  "t": {"type": "string", "maxLength": 120}},
                 "required": ["s", "t"]},
     [{"s": "ab", "t": ""}, {"s": "aébzz", "t": "hello world, this is a longer free string: with {braces} and [brackets]"}], True),
    ("numbers", {"type": "array", "items": {"type": "number"}, "minItems": 1, "maxItems": 3},
     [[0], [-1.5, 2e10, 3.25E-3], [12, 0.5]], True),
    ("arrays", {"type": "array", "items": {"type": "array", "items": {"type": "integer"}, "maxItems": 2}, "minItems": 2,
                "maxItems": 3},
     [[[], []], [[1, 2], [3], []]], True),
    ("nullable", {"type": ["string", "null"], "maxLength": 4}, [None, "abcd", ""], True),
    ("const", {"type": "object", "properties": {"kind": {"const": "pod"}, "n": {"const": 7}, "ok": {"const": True}},
               "required": ["kind", "n", "ok"]},
     [{"kind": "pod", "n": 7, "ok": True}], True),
    ("enum_mixed", {"enum": [1, 12, 123, "a", "ab", None, True, 2.5]}, [1, 12, 123, "a", "ab", None, True, 2.5], True),
    ("anyof", {"anyOf": [{"type": "integer"}, {"type": "string", "maxLength": 3}, {"type": "array", "items": {"type": "boolean"},
                                                                                 "maxItems": 2}, {"type": "null"}]},
     [5, "xy", [True, False], None], True),
    ("oneof_ref", {"$defs": {"name": {"type": "string", "minLength": 1, "maxLength": 8},
                             "pair": {"type": "object", "properties": {"k": {"$ref": "#/$defs/name"}, "v": {"type": "integer"}},
                                      "required": ["k"]}},
                   "type": "object",
                   "properties": {"items": {"type": "array", "items": {"$ref": "#/$defs/pair"}, "maxItems": 2},
                                  "pick": {"oneOf": [{"$ref": "#/$defs/name"}, {"type": "boolean"}]}},
                   "required": ["items", "pick"]},
     [{"items": [], "pick": "n"}, {"items": [{"k": "a", "v": 1}, {"k": "bb"}], "pick": False}], True),
    ("definitions", {"definitions": {"n": {"type": "integer"}}, "type": "array", "items": {"$ref": "#/definitions/n"},
                     "minItems": 2, "maxItems": 2}, [[1, -2]], True),
    ("closed", {"type": "object", "properties": {"o": {"type": "object", "additionalProperties": False},
                                                 "e": {"type": "array", "maxItems": 0}}, "required": ["o", "e"]},
     [{"o": {}, "e": []}], True),
    # free-form values: any JSON value / any object (a random walk through them need not end)
    ("free", {"type": "object", "properties": {"any": {}, "obj": {"type": "object"}, "list": {"type": "array", "maxItems": 2}},
              "required": ["any", "obj", "list"]},
     [{"any": {"a": [1, 2.5, "x", None, True, {"b": {}}]}, "obj": {"k": "v", "n": [0]}, "list": [1, "two"]},
      {"any": 17, "obj": {}, "list": []}], False),
]

REFUSED = [
    ("pattern", {"type": "string", "pattern": "^a"}),
    ("format", {"type": "string", "format": "date-time"}),
    ("minimum", {"type": "integer", "minimum": 0}),
    ("prefixItems", {"type": "array", "prefixItems": [{"type": "integer"}]}),
    ("not", {"not": {"type": "null"}}),
    ("$ref", {"$defs": {"node": {"type": "object", "properties": {"next": {"$ref": "#/$defs/node"}}}}, "$ref": "#/$defs/node"}),
    ("$ref", {"$ref": "http://example.com/schema.json"}),
    ("enum", {"enum": list(range(257))}),
    ("maxItems", {"type": "array", "maxItems": 4097}),
    ("maxLength", {"type": "string", "maxLength": 4097}),
    ("anyOf", {"anyOf": [{"type": "integer"}, {"type": "number"}]}),
    ("patternProperties", {"type": "object", "properties": {"a": {"patternProperties": {}}}}),
    ("64 KiB", {"enum": ["x" * 300 + str(i) for i in range(250)]}),
]


def compact(v) -> str:
    return json.dumps(v, separators=(",", ":"), ensure_ascii=False)


# ----------------------------------------------------------------------------- tokenizer stub
class StubTokenizer:
    """512 pieces: ids 0..94 the printable ASCII characters, then multi-character pieces,
    unused ids as U+FFFD (never allowed), id 511 end of sequence."""

    MULTI = ['{"', '":', '","', '":"', '"}', '",', "true", "false", "null", "list", "_pods", "get", "_logs", "scale",
             "_deployment", "cluster", "_context", "final", "_answer", "action", "replicas", "name", "10", "12", "100",
             '"action"', '{"action":"', "ab", "abc", "\\n", '\\"', "},", "],", "[[", "]]", '":[', "0.5", "e+"]

    def __init__(self):
        self.pieces = [chr(32 + i) for i in range(95)] + list(self.MULTI)
        self.pieces += ["�"] * (511 - len(self.pieces)) + [""]
        self.vocab_size = 512
        self.eos_ids = {511}

    def piece(self, i):
        return self.pieces[i]

    def decode(self, ids):
        return "".join(self.pieces[i] for i in ids if i not in self.eos_ids)


# ----------------------------------------------------------------------------- helpers
def random_walk(proc, eos_ids, rng: random.Random, max_steps: int = 400):
    """(ids, finished): a uniformly random allowed token per step until an end-of-sequence id."""
    ids = []
    for _ in range(max_steps):
        allowed = proc(ids).ids()
        t = int(allowed[rng.randrange(len(allowed))])
        if t in eos_ids:
            return ids, True
        ids.append(t)
    return ids, False


def pieces_by_text(tok) -> dict:
    out = {}
    for i in range(tok.vocab_size):
        t = tok.piece(i)
        if t and "�" not in t and i not in tok.eos_ids:
            out.setdefault(t, i)
    return out


def tokenise(proc, tok, text: str, by_text: dict):
    """``text`` as the engine would produce it: where the grammar forces the next piece, that
    piece; elsewhere the longest piece that is a prefix of the rest.  Asserts that the grammar
    allows every step, i.e. accepts every prefix.  -> (ids, forced steps)."""
    ids, pos, forced = [], 0, 0
    longest = max(len(t) for t in by_text)
    while pos < len(text):
        m = proc(ids)
        texts = {tok.piece(int(i)) for i in m.ids()} if len(m) <= 4 else None
        if texts is not None and len(texts) == 1:  # forced (duplicate pieces share one text)
            (piece,) = texts
            assert text.startswith(piece, pos), (text, pos, piece)
            t = int(m[0])
            forced += 1
        else:
            t = next(by_text[text[pos:pos + n]] for n in range(min(longest, len(text) - pos), 0, -1)
                     if text[pos:pos + n] in by_text)
            assert t in m, (text, pos, tok.piece(t))
        ids.append(t)
        pos += len(tok.piece(t))
    return ids, forced
