"""JSON-schema constrained decoding (docs/structured_outputs.md).

* :class:`TokenMask` -- an immutable allowed-token set as a bitmask (``uint32`` words, bit
  ``v & 31`` of word ``v >> 5`` is id ``v``).  The sampler keeps the masks it has seen in a device
  pool and applies them with one ``ops.mask_logits`` launch; to ``LLMEngine._jump`` a mask is a
  sequence (``len`` = set bits, ``mask[0]`` = lowest id).
* :class:`SchemaGrammar` -- a schema compiled to a character-level deterministic pushdown
  automaton over COMPACT JSON (no insignificant whitespace).  The allowed tokens of a state come
  from walking the tokenizer's piece trie through the automaton; masks are cached per state.
* :class:`SchemaCursor` -- one request's position in a shared grammar: the processor
  ``callable(output_ids) -> TokenMask`` that ``SamplingParams.logits_processor`` holds.

An automaton state is a tuple of frames, innermost last; ``()`` is "the value is complete".
"""
from __future__ import annotations

import json
from collections import OrderedDict
from typing import Optional

import numpy as np

from .constrained import JSON_START, WS, _J, _TokenTable, _num_ok, json_feed

MAX_DEPTH = 16          # nesting of objects / arrays, in the schema and inside free-form values
MAX_SCHEMA_BYTES = 64 << 10
MAX_ENUM = 256
MAX_COUNT = 4096        # maxItems / maxLength
MAX_INT_DIGITS = 18     # digits of a number's integer part and of its fraction
MAX_EXP_DIGITS = 3
MAX_MASKS = 4096        # cached masks per compiled grammar (number states of free-form values do not recur)

_ANNOTATIONS = {"title", "description", "default", "examples", "$schema", "$id", "$defs", "definitions"}
_KNOWN = _ANNOTATIONS | {"type", "properties", "required", "additionalProperties", "enum", "const", "minLength",
                         "maxLength", "items", "minItems", "maxItems", "anyOf", "oneOf", "$ref"}
_TYPES = ("null", "boolean", "integer", "number", "string", "array", "object")
_DIGITS = "0123456789"
_NUM_FIRST = "-" + _DIGITS
_ANY_FIRST = '{["tfn' + _NUM_FIRST
_HEX = "0123456789abcdefABCDEF"


def _dumps(v) -> str:
    return json.dumps(v, separators=(",", ":"), ensure_ascii=False)


# ----------------------------------------------------------------------------- token masks
class TokenMask:
    """Immutable allowed-token set: ``words`` (read-only ``uint32[ceil(vocab / 32)]``) and its
    popcount.  Identity is what the sampler's device pool keys on: a grammar hands out the same
    object every time a state recurs."""

    __slots__ = ("words", "count", "_ids")

    def __init__(self, words: np.ndarray):
        w = np.ascontiguousarray(words, dtype=np.uint32)
        w.setflags(write=False)
        self.words = w
        self.count = int(np.unpackbits(w.view(np.uint8)).sum())
        self._ids = None

    @classmethod
    def from_ids(cls, ids, vocab: int) -> "TokenMask":
        bits = np.zeros(-(-vocab // 32) * 32, dtype=np.uint8)
        a = np.asarray(ids, dtype=np.int64)
        bits[a[(a >= 0) & (a < vocab)]] = 1
        return cls(np.packbits(bits, bitorder="little").view(np.uint32))

    def ids(self) -> np.ndarray:
        """Sorted int64 array of the allowed ids."""
        if self._ids is None:
            a = np.flatnonzero(np.unpackbits(self.words.view(np.uint8), bitorder="little")).astype(np.int64)
            a.setflags(write=False)
            self._ids = a
        return self._ids

    def __len__(self) -> int:
        return self.count

    def __getitem__(self, i):
        return self.ids()[i]

    def __iter__(self):
        return iter(self.ids())

    def __contains__(self, t) -> bool:
        t = int(t)
        return 0 <= t < self.words.size * 32 and bool((int(self.words[t >> 5]) >> (t & 31)) & 1)


class _Pieces:
    """Per-tokenizer tables of the schema grammars: the piece trie (pieces with U+FFFD and
    end-of-sequence ids left out, ``_TokenTable``'s policy), the same trie over the pieces that
    are not plain string content, and the plain-content pieces' lengths."""

    _cache: dict = {}

    def __init__(self, tok):
        self.tok = tok
        tt = _TokenTable.get(tok)
        self.texts = tt.texts
        self.vocab = len(tt.texts)
        self.eos = list(tt.eos)
        # characters of each plain string-content piece (0: not one), padded to whole mask words
        self.plain_len = np.zeros(-(-self.vocab // 32) * 32, dtype=np.int32)
        for i in tt.plain_str:
            self.plain_len[i] = len(self.texts[i])
        self.special_trie = self._trie(tt.special)
        self.full_trie = self._trie(list(tt.plain_str) + list(tt.special))
        self.by_text: dict = {}
        for i in sorted(list(tt.plain_str) + list(tt.special)):
            self.by_text.setdefault(self.texts[i], []).append(i)
        self.lmax = max((len(t) for t in self.by_text), default=1)

    def _trie(self, ids):
        root = [{}, None]  # [children by character, ids whose piece ends here]
        for i in ids:
            node = root
            for ch in self.texts[i]:
                nxt = node[0].get(ch)
                if nxt is None:
                    nxt = node[0][ch] = [{}, None]
                node = nxt
            if node[1] is None:
                node[1] = []
            node[1].append(i)
        return root

    @classmethod
    def get(cls, tok) -> "_Pieces":
        hit = cls._cache.get(id(tok))
        if hit is None or hit.tok is not tok:
            hit = cls._cache[id(tok)] = cls(tok)
        return hit


# ----------------------------------------------------------------------------- schema -> nodes
def _refuse(keyword: str, why: str):
    raise ValueError(f"unsupported JSON schema: {keyword!r} {why}")


class _Compiler:
    """Schema -> node table.  Nodes: ("lits", lit id) | ("str", min, max) | ("num", is_int) |
    ("obj", props, lit ids per start index) | ("anyobj",) | ("arr", item, min, max) | ("any",) |
    ("union", {first char: node})."""

    def __init__(self, root: dict):
        self.root = root
        self.nodes: list = []
        self.first: list = []     # node -> characters a value of it can start with
        self.lits: list = []      # lit id -> {prefix: (complete, extendable, next characters, payload)}
        self._any = None

    def add(self, node, first) -> int:
        self.nodes.append(node)
        self.first.append(frozenset(first))
        return len(self.nodes) - 1

    def any(self) -> int:
        if self._any is None:
            self._any = self.add(("any",), _ANY_FIRST)
        return self._any

    def lit_table(self, texts: list, payloads: Optional[list] = None) -> int:
        tab: dict = {}
        for k, t in enumerate(texts):
            for n in range(len(t) + 1):
                e = tab.setdefault(t[:n], [False, set(), None])
                if n == len(t):
                    e[0] = True
                    e[2] = payloads[k] if payloads is not None else k
                else:
                    e[1].add(t[n])
        self.lits.append({p: (e[0], bool(e[1]), frozenset(e[1]), e[2]) for p, e in tab.items()})
        return len(self.lits) - 1

    def resolve(self, ref, active: tuple):
        if not isinstance(ref, str) or not (ref.startswith("#/$defs/") or ref.startswith("#/definitions/")):
            _refuse("$ref", f"must point into #/$defs or #/definitions, not {ref!r}")
        if ref in active:
            _refuse("$ref", f"is recursive ({ref})")
        _, group, name = ref.split("/", 2)
        name = name.replace("~1", "/").replace("~0", "~")
        defs = self.root.get(group) if isinstance(self.root, dict) else None
        if not isinstance(defs, dict) or name not in defs:
            _refuse("$ref", f"target {ref!r} does not exist")
        return defs[name]

    def compile(self, s, depth: int = 0, active: tuple = ()) -> int:
        if s is True:
            return self.any()
        if not isinstance(s, dict):
            _refuse("schema", f"must be an object or true, not {s!r}")
        for k in s:
            if k not in _KNOWN:
                _refuse(k, "is not a supported keyword")
        if depth > MAX_DEPTH:
            _refuse("properties", f"nest deeper than {MAX_DEPTH}")
        real = [k for k in s if k not in _ANNOTATIONS]
        if "$ref" in s:
            if len(real) > 1:
                _refuse("$ref", "cannot be combined with " + ", ".join(repr(k) for k in real if k != "$ref"))
            return self.compile(self.resolve(s["$ref"], active), depth, active + (s["$ref"],))
        for kw in ("anyOf", "oneOf"):
            if kw in s:
                if len(real) > 1:
                    _refuse(kw, "cannot be combined with " + ", ".join(repr(k) for k in real if k != kw))
                alts = s[kw]
                if not isinstance(alts, list) or not alts:
                    _refuse(kw, "must be a non-empty list")
                return self.union([self.compile(a, depth, active) for a in alts], kw)
        if "enum" in s or "const" in s:
            vals = list(s["enum"]) if "enum" in s and isinstance(s["enum"], list) else None
            if "enum" in s and vals is None:
                _refuse("enum", "must be a list")
            if vals is not None and len(vals) > MAX_ENUM:
                _refuse("enum", f"has more than {MAX_ENUM} values")
            if "const" in s:
                vals = [s["const"]] if vals is None else [v for v in vals if _same(v, s["const"])]
            for v in vals:
                if not (v is None or isinstance(v, (str, int, float, bool))) or (isinstance(v, float) and v != v):
                    _refuse("enum" if "enum" in s else "const", f"value {v!r} is not a scalar")
            if "type" in s:
                types = self.types(s["type"])
                vals = [v for v in vals if any(_is_type(v, t) for t in types)]
            for v in vals:  # the string keywords hold for the values too
                if isinstance(v, str) and not (int(s.get("minLength", 0)) <= len(v) <= int(s.get("maxLength", len(v)))):
                    vals = [x for x in vals if x is not v]
            texts = sorted({_dumps(v) for v in vals})
            if not texts:
                _refuse("enum" if "enum" in s else "const", "admits no value")
            return self.add(("lits", self.lit_table(texts)), {t[0] for t in texts})
        if "type" in s:
            types = self.types(s["type"])
        else:  # no type: the one the other keywords speak about, else any value
            types = [t for t, kws in (("object", ("properties", "required", "additionalProperties")),
                                      ("array", ("items", "minItems", "maxItems")),
                                      ("string", ("minLength", "maxLength"))) if any(k in s for k in kws)]
            if len(types) > 1:
                _refuse("type", "is missing and the other keywords speak about several types")
            if not types:
                return self.any()
        if "number" in types:
            types = [t for t in types if t != "integer"]
        return self.union([self.typed(t, s, depth, active) for t in types], "type")

    def types(self, t) -> list:
        ts = [t] if isinstance(t, str) else t
        if not isinstance(ts, list) or not ts or any(x not in _TYPES for x in ts):
            _refuse("type", f"must be one of {', '.join(_TYPES)} or a list of them, not {t!r}")
        return list(dict.fromkeys(ts))

    def union(self, alts: list, kw: str) -> int:
        if len(alts) == 1:
            return alts[0]
        table: dict = {}
        for a in alts:
            for ch in self.first[a]:
                if ch in table:
                    _refuse(kw, f"alternatives must start with distinct characters; two start with {ch!r}")
                table[ch] = a
        return self.add(("union", table), table)

    def bound(self, s: dict, lo_kw: str, hi_kw: str):
        lo, hi = s.get(lo_kw, 0), s.get(hi_kw)
        for kw, v in ((lo_kw, lo), (hi_kw, hi)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 0):
                _refuse(kw, f"must be a non-negative integer, not {v!r}")
        if hi is not None and hi > MAX_COUNT:
            _refuse(hi_kw, f"is above {MAX_COUNT}")
        if lo > MAX_COUNT:
            _refuse(lo_kw, f"is above {MAX_COUNT}")
        if hi is not None and lo > hi:
            _refuse(lo_kw, f"exceeds {hi_kw}")
        return lo, hi

    def typed(self, t: str, s: dict, depth: int, active: tuple) -> int:
        if t == "null":
            return self.add(("lits", self.lit_table(["null"])), "n")
        if t == "boolean":
            return self.add(("lits", self.lit_table(["false", "true"])), "tf")
        if t in ("integer", "number"):
            return self.add(("num", t == "integer"), _NUM_FIRST)
        if t == "string":
            lo, hi = self.bound(s, "minLength", "maxLength")
            return self.add(("str", lo, hi), '"')
        if t == "array":
            lo, hi = self.bound(s, "minItems", "maxItems")
            item = self.compile(s["items"], depth + 1, active) if "items" in s else self.any()
            return self.add(("arr", item, lo, hi), "[")
        # object
        req = s.get("required", [])
        if not isinstance(req, list) or any(not isinstance(r, str) for r in req):
            _refuse("required", "must be a list of names")
        ap = s.get("additionalProperties")
        if "properties" not in s:
            if req:
                _refuse("required", "needs 'properties' that declare the names")
            if ap is False:
                return self.add(("lits", self.lit_table(["{}"])), "{")
            if ap not in (None, True, {}):
                _refuse("additionalProperties", "with a schema is not supported")
            return self.add(("anyobj",), "{")
        props = s["properties"]
        if not isinstance(props, dict):
            _refuse("properties", "must be an object")
        if ap is not None and not isinstance(ap, (bool, dict)):
            _refuse("additionalProperties", "must be a boolean or a schema")
        for r in req:
            if r not in props:
                _refuse("required", f"names {r!r}, which 'properties' does not declare")
        plist = [(_dumps(k) + ":", self.compile(v, depth + 1, active), k in req) for k, v in props.items()]
        # start index i -> the keys that may come next: up to and including the first required one
        tabs = []
        for i in range(len(plist) + 1):
            cand = []
            for j in range(i, len(plist)):
                cand.append(j)
                if plist[j][2]:
                    break
            tabs.append(self.lit_table([plist[j][0] for j in cand], cand) if cand else None)
        closable = [not any(p[2] for p in plist[i:]) for i in range(len(plist) + 1)]
        return self.add(("obj", plist, tabs, closable), "{")


def _same(a, b) -> bool:
    return type(a) is type(b) and a == b or (not isinstance(a, bool) and not isinstance(b, bool)
                                             and isinstance(a, (int, float)) and isinstance(b, (int, float)) and a == b)


def _is_type(v, t: str) -> bool:
    if t == "null":
        return v is None
    if t == "boolean":
        return isinstance(v, bool)
    if t == "string":
        return isinstance(v, str)
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        return False
    return t == "number" or (t == "integer" and (isinstance(v, int) or float(v).is_integer()))


# ----------------------------------------------------------------------------- the grammar
class SchemaGrammar:
    """Compiled schema + per-state :class:`TokenMask` cache, shared by every request with the
    same (tokenizer, schema): see :func:`compiled`.  Raises ``ValueError`` naming the keyword
    for anything outside the supported subset."""

    def __init__(self, tok, schema):
        if schema is True:
            schema = {}
        if not isinstance(schema, dict):
            raise ValueError("unsupported JSON schema: the schema must be an object")
        canon = _dumps(schema)
        if len(canon.encode()) > MAX_SCHEMA_BYTES:
            raise ValueError(f"unsupported JSON schema: the schema is larger than {MAX_SCHEMA_BYTES >> 10} KiB")
        c = _Compiler(schema)
        self.root = c.compile(schema)
        self.nodes, self.first, self.lits = c.nodes, c.first, c.lits
        self.tok = tok
        self.pc = _Pieces.get(tok)
        self.vocab = self.pc.vocab
        self.start = (("V", self.root),)
        self.masks: dict = {}
        self.mask_builds = 0  # masks computed (cache misses), for tests and docs
        self._end = TokenMask.from_ids(self.pc.eos or [0], self.vocab)

    # ---- the automaton
    def feed(self, st: tuple, ch: str):
        """State after one more character, or None if ``ch`` cannot come next."""
        if not st:
            return None
        top = st[-1]
        rest = st[:-1]
        k = top[0]
        if k == "V":
            return self._begin(top[1], ch, rest)
        if k == "S":
            _, need, room, mode = top
            if mode == 0:
                if ch == '"':
                    return rest if need == 0 else None
                if ord(ch) < 0x20 or room == 0:
                    return None
                return rest + (("S", need - 1 if need else 0, room - 1 if room is not None else None,
                                1 if ch == "\\" else 0),)
            if mode == 1:  # after a backslash (the escape counted as one character at the backslash)
                if ch in '"\\/bfnrt':
                    return rest + (("S", need, room, 0),)
                return rest + (("S", need, room, 2),) if ch == "u" else None
            if ch not in _HEX:
                return None
            if mode == 2:  # \uD8xx-\uDFxx (half of a surrogate pair) is not a character: refused
                return rest + (("S", need, room, 6 if ch in "dD" else 3),)
            if mode == 6:
                return None if ch in "89abcdefABCDEF" else rest + (("S", need, room, 4),)
            return rest + (("S", need, room, 0 if mode == 5 else mode + 1),)
        if k == "L":
            _, lid, prefix = top
            tab = self.lits[lid]
            e = tab.get(prefix + ch)
            if e is None:  # a complete value that a longer one extends (1 / 12) ends at a character of the parent
                return self.feed(rest, ch) if tab[prefix][0] else None
            if e[0] and not e[1]:
                return rest
            return rest + (("L", lid, prefix + ch),)
        if k == "K":
            _, nid, i, prefix = top
            node = self.nodes[nid]
            e = self.lits[node[2][i]].get(prefix + ch)
            if e is None:
                return None
            if e[0]:
                j = e[3]
                return rest + (("O", nid, j + 1, 1), ("V", node[1][j][1]))
            return rest + (("K", nid, i, prefix + ch),)
        if k == "O":
            _, nid, i, phase = top
            node = self.nodes[nid]
            if ch == '"' and phase != 1 and node[2][i] is not None:
                return rest + (("K", nid, i, '"'),)
            if ch == "," and phase == 1 and node[2][i] is not None:
                return rest + (("O", nid, i, 2),)
            if ch == "}" and phase != 2 and node[3][i]:
                return rest
            return None
        if k == "A":
            _, nid, need, room, phase = top
            item = self.nodes[nid][1]
            if phase == 1:
                if ch == "," and room != 0:
                    return rest + (("A", nid, need, room, 2),)
                return rest if ch == "]" and need == 0 else None
            if phase == 0 and ch == "]":
                return rest if need == 0 else None
            if room == 0:
                return None
            return self._begin(item, ch, rest + (("A", nid, need - 1 if need else 0,
                                                  room - 1 if room is not None else None, 1),))
        if k == "N":
            _, is_int, s, n = top
            if ch in _DIGITS:
                if s <= 1:
                    return rest + (("N", is_int, 2 if ch == "0" else 3, 1),)
                if s == 2:
                    return None
                if s in (3, 5, 8):
                    if n >= (MAX_EXP_DIGITS if s == 8 else MAX_INT_DIGITS):
                        return None
                    return rest + (("N", is_int, s, n + 1),)
                return rest + (("N", is_int, {4: 5, 6: 8, 7: 8}[s], 1),)
            if ch == "-" and s == 0:
                return rest + (("N", is_int, 1, 0),)
            if not is_int:
                if ch == "." and s in (2, 3):
                    return rest + (("N", False, 4, 0),)
                if ch in "eE" and s in (2, 3, 5):
                    return rest + (("N", False, 6, 0),)
                if ch in "+-" and s == 6:
                    return rest + (("N", False, 7, 0),)
            return self.feed(rest, ch) if s in (2, 3, 5, 8) else None  # a complete number ends at the parent's character
        if k == "J":
            jst = top[1]
            mode = jst[0]
            if ch in WS and mode != _J.STR:
                return None
            if mode == _J.NUM and not jst[1] and ch not in "0123456789+-.eE":
                return self.feed(rest, ch) if _num_ok(jst[2], True) else None
            nxt = json_feed(jst, ch)
            if nxt is None or len(nxt[1]) > MAX_DEPTH:
                return None
            return rest if nxt[0] == _J.DONE else rest + (("J", nxt),)
        return None

    def _begin(self, nid: int, ch: str, rest: tuple):
        """State after the first character ``ch`` of a value of node ``nid``."""
        node = self.nodes[nid]
        k = node[0]
        if ch not in self.first[nid]:
            return None
        if k == "union":
            return self._begin(node[1][ch], ch, rest)
        if k == "lits":
            e = self.lits[node[1]][ch]
            return rest if e[0] and not e[1] else rest + (("L", node[1], ch),)
        if k == "str":
            return rest + (("S", node[1], node[2], 0),)
        if k == "num":
            return rest + (("N", node[1], 1, 0) if ch == "-" else ("N", node[1], 2 if ch == "0" else 3, 1),)
        if k == "obj":
            return rest + (("O", nid, 0, 0),)
        if k == "arr":
            return rest + (("A", nid, node[2], node[3], 0),)
        return rest + (("J", json_feed(JSON_START, ch)),)  # any / anyobj

    def feed_text(self, st, text: str):
        for ch in text:
            st = self.feed(st, ch)
            if st is None:
                return None
        return st

    def final(self, st) -> bool:
        """The text so far is a complete value (a top-level number also is while it may go on)."""
        if st is None:
            return False
        if not st:
            return True
        if len(st) > 1:
            return False
        top = st[0]
        if top[0] == "N":
            return top[2] in (2, 3, 5, 8)
        if top[0] == "L":
            return self.lits[top[1]][top[2]][0]
        return top[0] == "J" and top[1][0] == _J.NUM and _num_ok(top[1][2], True)

    def advance(self, st, token: int):
        """State after a generated token (end-of-sequence ids leave it where it is)."""
        if st is None or token in self.pc.eos:
            return st
        text = self.pc.texts[token] if 0 <= token < self.vocab else ""
        return self.feed_text(st, text) if text else None

    # ---- forced runs
    def _next_chars(self, st):
        """The characters that can come next when they are few (structure, literals), else None."""
        top = st[-1]
        k = top[0]
        if k == "V":
            return self.first[top[1]]
        if k == "L":
            e = self.lits[top[1]][top[2]]
            return None if e[0] else e[2]
        if k == "K":
            return self.lits[self.nodes[top[1]][2][top[2]]][top[3]][2]
        if k == "O":
            _, nid, i, phase = top
            node = self.nodes[nid]
            out = set()
            if node[2][i] is not None:
                out.add("," if phase == 1 else '"')
            if phase != 2 and node[3][i]:
                out.add("}")
            return out
        if k == "A":
            _, nid, need, room, phase = top
            if phase == 1:
                return ({","} if room != 0 else set()) | ({"]"} if need == 0 else set())
            out = set(self.first[self.nodes[nid][1]]) if room != 0 else set()
            if phase == 0 and need == 0:
                out.add("]")
            return out
        if k == "S" and top[3] == 0 and top[2] == 0 and top[1] == 0:
            return {'"'}  # a string at its maxLength can only close
        return None

    def forced_run(self, st) -> str:
        """The characters that must come next (at most as many as the longest piece has)."""
        run = []
        while st and len(run) < self.pc.lmax:
            nc = self._next_chars(st)
            if nc is None or len(nc) != 1:
                break
            (ch,) = nc
            st = self.feed(st, ch)
            run.append(ch)
        return "".join(run)

    # ---- masks
    def _key(self, st: tuple) -> tuple:
        """``st`` with every counter clamped just beyond the reach of one piece: states further
        than that from a limit allow the same tokens (maxLength 200 is not 200 masks)."""
        cap = self.pc.lmax + 1
        out = []
        for f in st:
            if f[0] == "S":
                f = ("S", min(f[1], cap), None if f[2] is None else min(f[2], cap), f[3])
            elif f[0] == "A":
                f = ("A", f[1], min(f[2], cap), None if f[3] is None else min(f[3], cap), f[4])
            out.append(f)
        return tuple(out)

    def mask(self, st) -> TokenMask:
        """Allowed next tokens of state ``st`` (None = the text left the grammar: end only)."""
        if not st:
            return self._end
        key = self._key(st)
        hit = self.masks.get(key)
        if hit is not None:
            return hit
        self.mask_builds += 1
        pc = self.pc
        ids = None
        run = self.forced_run(st)
        for n in range(len(run), 0, -1):  # forced: the longest piece spelling a prefix of the run
            ids = pc.by_text.get(run[:n])
            if ids:
                break
        if ids:
            m = TokenMask.from_ids(ids, self.vocab)
        else:
            top = st[-1]
            free = (top[0] == "S" and top[3] == 0) or (top[0] == "J" and top[1][0] == _J.STR)
            # inside a string every plain piece that fits stays inside it: only the pieces with
            # a quote, a backslash or a control character are walked
            if free:
                room = top[2] if top[0] == "S" and top[2] is not None else pc.lmax
                bits = ((pc.plain_len > 0) & (pc.plain_len <= room)).astype(np.uint8)
            else:
                bits = np.zeros(pc.plain_len.size, dtype=np.uint8)
            got = self._walk(st, pc.special_trie if free else pc.full_trie)
            if self.final(st):
                got += pc.eos
            if got:
                bits[np.asarray(got, dtype=np.int64)] = 1
            if not bits.any():  # no piece fits (a vocabulary without the character): end
                return self._end
            m = TokenMask(np.packbits(bits, bitorder="little").view(np.uint32))
        if len(self.masks) < MAX_MASKS:
            self.masks[key] = m
        return m

    def _walk(self, st, trie) -> list:
        out = []
        feed = self.feed
        todo = [(trie, st)]
        while todo:
            node, s = todo.pop()
            for ch, child in node[0].items():
                s2 = feed(s, ch)
                if s2 is None:
                    continue
                if child[1] is not None:
                    out += child[1]
                if child[0] and s2:
                    todo.append((child, s2))
        return out

    def cursor(self) -> "SchemaCursor":
        return SchemaCursor(self)


class SchemaCursor:
    """One request's processor over a shared :class:`SchemaGrammar`: ``cursor(output_ids)`` is
    the :class:`TokenMask` of the state after ``output_ids``.  It advances from the longest
    prefix of ``output_ids`` it has already consumed (the same ids again, ids several tokens
    longer after a jump-forward) and starts over where the ids diverge."""

    def __init__(self, grammar: SchemaGrammar):
        self.grammar = grammar
        self._ids: list = []
        self._states: list = [grammar.start]  # _states[k]: after k tokens

    def state_after(self, ids):
        g = self.grammar
        mine = self._ids
        n = len(ids)
        k = len(mine)
        if k > n or ids[:k] != mine:
            k = 0
            lim = min(n, len(mine))
            while k < lim and ids[k] == mine[k]:
                k += 1
            del mine[k:]
            del self._states[k + 1:]
        st = self._states[k]
        for t in ids[k:]:
            st = g.advance(st, int(t))
            mine.append(int(t))
            self._states.append(st)
        return st

    def __call__(self, ids) -> TokenMask:
        return self.grammar.mask(self.state_after(list(ids)))


# compiled grammars by (tokenizer, canonical schema JSON; key order kept, it is the emission
# order): concurrent requests with one schema share
# the TokenMask objects, and through them the rows of the sampler's device pool
_COMPILED: "OrderedDict" = OrderedDict()
COMPILED_MAX = 32


def compiled(tok, schema) -> SchemaGrammar:
    if schema is True:
        schema = {}
    if not isinstance(schema, dict):
        raise ValueError("unsupported JSON schema: the schema must be an object")
    canon = _dumps(schema)
    key = (id(tok), canon)
    hit = _COMPILED.get(key)
    if hit is not None and hit.tok is tok:
        _COMPILED.move_to_end(key)
        return hit
    g = SchemaGrammar(tok, schema)
    _COMPILED[key] = g
    while len(_COMPILED) > COMPILED_MAX:
        _COMPILED.popitem(last=False)
    return g
