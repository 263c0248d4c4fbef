"""Grammar compiler: regex subset, choice lists and a JSON-schema subset to byte-level DFAs.

A compiled grammar is a DFA over UTF-8 bytes:

* ``trans`` uint16 ``[S, 256]``: state 0 is dead (all its transitions are 0), state 1 is the
  start state;
* ``accept`` uint8 ``[S]``.

States from which no accepting state can be reached are removed, so a live state is accepting
or has a continuation. No DFA accepts ill-formed UTF-8: ``.``, negated classes and
``\\D \\W \\S`` are compiled to the byte sequences of exactly one Unicode scalar value
(no overlong forms, no surrogates, nothing above U+10FFFF).

Pipeline: pattern -> AST -> Thompson NFA with byte-range edges -> subset construction over
byte equivalence classes (the ranges' boundaries split 0..255 into a few dozen classes, so a
DFA state costs one closure per class, not 256) -> trim -> dense table.

JSON whitespace policy (one policy that cannot loop): no whitespace anywhere except at most
one space after ``:`` and after ``,``.
"""
from __future__ import annotations

import json
import threading
from collections import OrderedDict
from typing import Optional

import numpy as np

MAX_STATES = 8192          # default per-grammar cap
HARD_MAX_STATES = 65535    # what uint16 holds
MAX_CP = 0x10FFFF

# ---------------------------------------------------------------- AST
# ("set", ((lo, hi), ...))  one scalar value out of sorted disjoint code-point ranges
# ("cat", [nodes])   ("alt", [nodes])   ("rep", node, m, n or None)


def _norm(ranges):
    out = []
    for lo, hi in sorted(ranges):
        if lo > hi:
            continue
        if out and lo <= out[-1][1] + 1:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return tuple(out)


def _negate(ranges):
    out, prev = [], 0
    for lo, hi in _norm(ranges):
        if lo > prev:
            out.append((prev, lo - 1))
        prev = hi + 1
    if prev <= MAX_CP:
        out.append((prev, MAX_CP))
    return tuple(out)


def cset(ranges, negate=False):
    r = _negate(ranges) if negate else _norm(ranges)
    if not r:
        raise ValueError("empty character class")
    return ("set", r)


def lit(s: str):
    return ("cat", [("set", ((ord(c), ord(c)),)) for c in s])


_DIGIT = ((48, 57),)
_WORD = ((48, 57), (65, 90), (95, 95), (97, 122))
_SPACE = ((9, 13), (32, 32))
_ESC_CLASS = {"d": _DIGIT, "w": _WORD, "s": _SPACE}
_ESC_CHAR = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11, "0": 0}


class _Parser:
    """Recursive descent over the supported subset; everything else raises ValueError."""

    def __init__(self, pat: str):
        self.p, self.i = pat, 0

    def err(self, msg):
        return ValueError(f"regex: {msg} at offset {self.i} of {self.p!r}")

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        if self.peek() == "^":
            self.i += 1
        node = self.alt()
        if self.i < len(self.p):
            raise self.err("unbalanced ')'")
        return node

    def alt(self):
        items = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            items.append(self.cat())
        return items[0] if len(items) == 1 else ("alt", items)

    def cat(self):
        items = []
        while True:
            c = self.peek()
            if c is None or c in "|)":
                break
            if c == "$":
                rest = self.p[self.i + 1:]
                if all(ch == ")" for ch in rest):  # before the closing brackets of the outermost groups only
                    self.i += 1
                    continue
                raise self.err("'$' is supported only at the end")
            if c == "^":
                raise self.err("'^' is supported only at the start")
            items.append(self.repeat(self.atom()))
        return ("cat", items)

    def repeat(self, node):
        while True:
            c = self.peek()
            if c == "*":
                m, n = 0, None
            elif c == "+":
                m, n = 1, None
            elif c == "?":
                m, n = 0, 1
            elif c == "{":
                j = self.p.find("}", self.i)
                if j < 0:
                    raise self.err("unterminated '{'")
                body = self.p[self.i + 1:j]
                parts = body.split(",")
                try:
                    if len(parts) == 1:
                        m = n = int(parts[0])
                    elif len(parts) == 2:
                        m = int(parts[0])
                        n = int(parts[1]) if parts[1] != "" else None
                    else:
                        raise ValueError
                    if not all(x.isdigit() for x in parts if x != "") or parts[0] == "":
                        raise ValueError
                except ValueError:
                    raise self.err("bad quantifier {%s}" % body) from None
                if n is not None and n < m:
                    raise self.err("bad quantifier range")
                self.i = j
            else:
                return node
            self.i += 1
            if self.peek() in ("?", "+"):
                raise self.err("lazy and possessive quantifiers are not supported")
            node = ("rep", node, m, n)

    def atom(self):
        c = self.peek()
        self.i += 1
        if c == "(":
            if self.peek() == "?":
                if self.p[self.i:self.i + 2] == "?:":
                    self.i += 2
                else:
                    raise self.err("look-around, named groups and inline flags are not supported")
            node = self.alt()
            if self.peek() != ")":
                raise self.err("missing ')'")
            self.i += 1
            return node
        if c == "[":
            return self.klass()
        if c == ".":
            return cset(((10, 10),), negate=True)
        if c == "\\":
            r = self.escape()
            return ("set", r)
        if c in "*+?{":
            raise self.err("nothing to repeat")
        if c in "]}":
            raise self.err(f"unescaped {c!r}")
        return ("set", ((ord(c), ord(c)),))

    def escape(self):
        c = self.peek()
        if c is None:
            raise self.err("trailing backslash")
        self.i += 1
        if c in _ESC_CLASS:
            return _ESC_CLASS[c]
        if c in "DWS":
            return _negate(_ESC_CLASS[c.lower()])
        if c in _ESC_CHAR:
            return ((_ESC_CHAR[c], _ESC_CHAR[c]),)
        if c == "x":
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or any(ch not in "0123456789abcdefABCDEF" for ch in h):
                raise self.err("bad \\x escape")
            self.i += 2
            return ((int(h, 16), int(h, 16)),)
        if c == "u":
            h = self.p[self.i:self.i + 4]
            if len(h) != 4 or any(ch not in "0123456789abcdefABCDEF" for ch in h):
                raise self.err("bad \\u escape")
            self.i += 4
            return ((int(h, 16), int(h, 16)),)
        if c.isdigit():
            raise self.err("backreferences are not supported")
        if c.isalnum():
            raise self.err(f"unsupported escape \\{c}")
        return ((ord(c), ord(c)),)

    def klass(self):
        neg = False
        if self.peek() == "^":
            neg = True
            self.i += 1
        ranges, first = [], True
        while True:
            c = self.peek()
            if c is None:
                raise self.err("unterminated character class")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            self.i += 1
            if c == "\\":
                r = self.escape()
            else:
                r = ((ord(c), ord(c)),)
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                if len(r) != 1 or r[0][0] != r[0][1]:
                    raise self.err("bad range in character class")
                self.i += 1
                d = self.peek()
                self.i += 1
                if d == "\\":
                    r2 = self.escape()
                    if len(r2) != 1 or r2[0][0] != r2[0][1]:
                        raise self.err("bad range in character class")
                    hi = r2[0][0]
                else:
                    hi = ord(d)
                if hi < r[0][0]:
                    raise self.err("reversed range in character class")
                r = ((r[0][0], hi),)
            ranges.extend(r)
        try:
            return cset(ranges, negate=neg)
        except ValueError:
            raise self.err("empty character class") from None


def parse_regex(pattern: str):
    if not isinstance(pattern, str):
        raise ValueError("regex must be a string")
    return _Parser(pattern).parse()


# ---------------------------------------------------------------- UTF-8 byte sequences of a code-point range
def _enc(cp: int) -> bytes:
    return chr(cp).encode("utf-8")


def _utf8_seqs(lo: int, hi: int, out: list):
    """Append byte-range sequences [(lo, hi), ...] whose product is exactly the UTF-8 encodings
    of the scalar values in [lo, hi] (surrogates left out)."""
    if lo > hi:
        return
    if lo <= 0xDFFF and hi >= 0xD800:  # surrogates are no scalar values
        _utf8_seqs(lo, 0xD7FF, out)
        _utf8_seqs(0xE000, hi, out)
        return
    for mx in (0x7F, 0x7FF, 0xFFFF):
        if lo <= mx < hi:
            _utf8_seqs(lo, mx, out)
            _utf8_seqs(mx + 1, hi, out)
            return
    if hi <= 0x7F:
        out.append([(lo, hi)])
        return
    for i in range(1, 4):
        m = (1 << (6 * i)) - 1
        if (lo & ~m) != (hi & ~m):
            if lo & m:
                _utf8_seqs(lo, lo | m, out)
                _utf8_seqs((lo | m) + 1, hi, out)
                return
            if (hi & m) != m:
                _utf8_seqs(lo, (hi & ~m) - 1, out)
                _utf8_seqs(hi & ~m, hi, out)
                return
    a, b = _enc(lo), _enc(hi)
    out.append(list(zip(a, b)))


# ---------------------------------------------------------------- NFA
class _NFA:
    def __init__(self):
        self.eps: list[list[int]] = []
        self.edges: list[list[tuple[int, int, int]]] = []  # (byte lo, byte hi, target)

    def new(self) -> int:
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node, limit: int) -> tuple[int, int]:
        """Fragment (start, end) of ``node``."""
        if len(self.eps) > limit:
            raise ValueError("grammar too large")
        kind = node[0]
        if kind == "set":
            s, e = self.new(), self.new()
            seqs: list = []
            for lo, hi in node[1]:
                _utf8_seqs(lo, hi, seqs)
            # sequences that continue with the same byte ranges share that tail
            tails: dict = {(): e}
            for seq in seqs:
                cur = s
                for k, (bl, bh) in enumerate(seq):
                    rest = tuple(seq[k + 1:])
                    nxt = tails.get(rest)
                    known = nxt is not None
                    if not known:
                        nxt = tails[rest] = self.new()
                    self.edges[cur].append((bl, bh, nxt))
                    if known:
                        break
                    cur = nxt
            return s, e
        if kind == "cat":
            s = e = self.new()
            for it in node[1]:
                a, b = self.build(it, limit)
                self.eps[e].append(a)
                e = b
            return s, e
        if kind == "alt":
            s, e = self.new(), self.new()
            for it in node[1]:
                a, b = self.build(it, limit)
                self.eps[s].append(a)
                self.eps[b].append(e)
            return s, e
        if kind == "rep":
            _, sub, m, n = node
            s = e = self.new()
            for _ in range(m):
                a, b = self.build(sub, limit)
                self.eps[e].append(a)
                e = b
            if n is None:
                a, b = self.build(sub, limit)
                loop = self.new()
                self.eps[e].append(loop)
                self.eps[loop].append(a)
                self.eps[b].append(loop)
                e = loop
            else:
                end = self.new()
                for _ in range(n - m):
                    self.eps[e].append(end)
                    a, b = self.build(sub, limit)
                    self.eps[e].append(a)
                    e = b
                self.eps[e].append(end)
                e = end
            return s, e
        raise AssertionError(kind)


class Grammar:
    """A compiled DFA; immutable, shared between requests and cached."""

    _uid = 0
    _uid_lock = threading.Lock()

    def __init__(self, kind: str, key: str, trans: np.ndarray, accept: np.ndarray):
        assert trans.dtype == np.uint16 and trans.ndim == 2 and trans.shape[1] == 256
        assert accept.dtype == np.uint8 and accept.shape == (trans.shape[0],)
        self.kind, self.key = kind, key
        self.trans, self.accept = trans, accept
        self.num_states = int(trans.shape[0])
        with Grammar._uid_lock:
            Grammar._uid += 1
            self.uid = Grammar._uid

    def advance(self, state: int, data: bytes) -> int:
        t = self.trans
        for b in data:
            state = int(t[state, b])
            if state == 0:
                break
        return state

    def accepts(self, data: bytes) -> bool:
        return bool(self.accept[self.advance(1, data)])

    def is_accepting(self, state: int) -> bool:
        return bool(self.accept[state])

    def __repr__(self):
        return f"Grammar({self.kind}, {self.num_states} states)"


def _nfa_to_grammar(nfa: _NFA, start: int, end: int, kind: str, key: str, max_states: int) -> Grammar:
    # byte equivalence classes from the edges' boundaries
    cuts = {0, 256}
    for es in nfa.edges:
        for lo, hi, _ in es:
            cuts.add(lo)
            cuts.add(hi + 1)
    bounds = sorted(cuts)
    cls_of = np.zeros(256, dtype=np.int64)
    reps = []
    for c, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        cls_of[a:b] = c
        reps.append(a)
    ncls = len(reps)
    # per NFA state: class -> targets
    N = len(nfa.eps)
    step: list[dict] = [dict() for _ in range(N)]
    for s, es in enumerate(nfa.edges):
        for lo, hi, t in es:
            for c in range(int(cls_of[lo]), int(cls_of[hi]) + 1):
                step[s].setdefault(c, []).append(t)
    clo_cache: dict[int, frozenset] = {}

    def closure1(s):
        r = clo_cache.get(s)
        if r is None:
            seen, stack = {s}, [s]
            while stack:
                x = stack.pop()
                for y in nfa.eps[x]:
                    if y not in seen:
                        seen.add(y)
                        stack.append(y)
            # only states that matter afterwards: those with byte edges, and the end
            r = clo_cache[s] = frozenset(x for x in seen if nfa.edges[x] or x == end)
        return r

    start_set = closure1(start)
    ids = {start_set: 0}
    sets = [start_set]
    rows: list[list[int]] = []
    k = 0
    while k < len(sets):
        cur = sets[k]
        k += 1
        by_cls: dict[int, set] = {}
        for s in cur:
            for c, ts in step[s].items():
                by_cls.setdefault(c, set()).update(ts)
        row = [-1] * ncls
        for c, ts in by_cls.items():
            nxt = frozenset().union(*[closure1(t) for t in ts])
            j = ids.get(nxt)
            if j is None:
                j = ids[nxt] = len(sets)
                sets.append(nxt)
                if len(sets) + 1 > max_states:
                    raise ValueError(f"grammar needs more than {max_states} DFA states")
            row[c] = j
        rows.append(row)
    S = len(sets)
    tc = np.asarray(rows, dtype=np.int64).reshape(S, ncls)
    acc = np.fromiter((end in st for st in sets), dtype=bool, count=S)
    # trim: keep the states that reach an accepting one
    live = acc.copy()
    while True:
        nxt_live = np.concatenate([live, [False]])[tc].any(axis=1) | live  # index -1 -> False
        if (nxt_live == live).all():
            break
        live = nxt_live
    if not live[0]:
        raise ValueError("grammar matches nothing")
    # reachable from the start through live states only, numbered from 1 in BFS order
    order, new_id, q = [0], {0: 1}, [0]
    while q:
        x = q.pop(0)
        for y in tc[x]:
            y = int(y)
            if y >= 0 and live[y] and y not in new_id:
                new_id[y] = len(order) + 1
                order.append(y)
                q.append(y)
    n = len(order) + 1
    if n > min(max_states, HARD_MAX_STATES):
        raise ValueError(f"grammar needs more than {max_states} DFA states")
    remap = np.zeros(S + 1, dtype=np.uint16)  # slot S: the missing transition (-1)
    for old, new in new_id.items():
        remap[old] = new
    tcls = np.zeros((n, ncls), dtype=np.uint16)
    tcls[1:] = remap[tc[order]]
    trans = np.ascontiguousarray(tcls[:, cls_of])
    accept = np.zeros(n, dtype=np.uint8)
    accept[1:] = acc[order]
    return Grammar(kind, key, trans, accept)


def _compile_ast(ast, kind, key, max_states) -> Grammar:
    max_states = _cap(max_states)
    nfa = _NFA()
    s, e = nfa.build(ast, limit=64 * max_states + 4096)
    return _nfa_to_grammar(nfa, s, e, kind, key, max_states)


def _cap(max_states: Optional[int]) -> int:
    m = MAX_STATES if max_states is None else int(max_states)
    if m < 2:
        raise ValueError("max_states must be at least 2")
    return min(m, HARD_MAX_STATES)


def compile_regex(pattern: str, max_states: Optional[int] = None) -> Grammar:
    return _compile_ast(parse_regex(pattern), "regex", pattern, max_states)


def compile_choice(choices, max_states: Optional[int] = None) -> Grammar:
    """Trie DFA of a non-empty list of non-empty strings."""
    if not isinstance(choices, (list, tuple)) or not choices:
        raise ValueError("guided_choice must be a non-empty list of strings")
    cap = _cap(max_states)
    rows = [np.zeros(256, dtype=np.uint16), np.zeros(256, dtype=np.uint16)]
    acc = [0, 0]
    for c in choices:
        if not isinstance(c, str) or not c:
            raise ValueError("guided_choice entries must be non-empty strings")
        s = 1
        for b in c.encode("utf-8"):
            t = int(rows[s][b])
            if t == 0:
                t = len(rows)
                if t + 1 > cap:
                    raise ValueError(f"grammar needs more than {cap} DFA states")
                rows.append(np.zeros(256, dtype=np.uint16))
                acc.append(0)
                rows[s][b] = t
            s = t
        acc[s] = 1
    return Grammar("choice", json.dumps(list(choices)), np.stack(rows), np.asarray(acc, dtype=np.uint8))


# ---------------------------------------------------------------- JSON schema
_ANNOTATIONS = {"title", "description", "default", "examples", "$schema", "$id", "$comment", "$defs",
                "definitions"}
_STRING_CHAR = ("alt", [cset(((0x00, 0x1F), (0x22, 0x22), (0x5C, 0x5C)), negate=True),
                        parse_regex(r'\\(["\\/bfnrt]|u[0-9a-fA-F]{4})')])
_INTEGER = parse_regex(r"-?(0|[1-9][0-9]*)")
_NUMBER = parse_regex(r"-?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?")
_SP = ("rep", lit(" "), 0, 1)  # the whitespace policy: at most one space after ':' and ','


def _json_lit(v):
    return lit(json.dumps(v, ensure_ascii=False, separators=(",", ":")))


def _schema_ast(sch, root, stack: tuple):
    if sch is True or not isinstance(sch, dict):
        raise ValueError("unsupported JSON schema: expected an object describing a type "
                         "(a general JSON grammar is out of scope)")
    allowed = set(_ANNOTATIONS)

    def check(extra):
        bad = set(sch) - allowed - set(extra)
        if bad:
            raise ValueError(f"unsupported JSON schema keyword(s): {sorted(bad)}")

    if "$ref" in sch:
        check({"$ref"})
        ref = sch["$ref"]
        if not isinstance(ref, str) or not (ref.startswith("#/$defs/") or ref.startswith("#/definitions/")):
            raise ValueError(f"unsupported $ref {ref!r}: only #/$defs/NAME and #/definitions/NAME")
        if ref in stack:
            raise ValueError(f"recursive $ref {ref!r} is not supported")
        _, table, name = ref.split("/", 2)
        target = (root.get(table) or {}).get(name) if isinstance(root, dict) else None
        if target is None:
            raise ValueError(f"unresolved $ref {ref!r}")
        return _schema_ast(target, root, stack + (ref,))
    if "enum" in sch:
        check({"enum", "type"})
        if not isinstance(sch["enum"], list) or not sch["enum"]:
            raise ValueError("enum must be a non-empty list")
        return ("alt", [_json_lit(v) for v in sch["enum"]])
    if "const" in sch:
        check({"const", "type"})
        return _json_lit(sch["const"])
    for k in ("anyOf", "oneOf"):
        if k in sch:
            check({k})
            if not isinstance(sch[k], list) or not sch[k]:
                raise ValueError(f"{k} must be a non-empty list")
            return ("alt", [_schema_ast(s, root, stack) for s in sch[k]])
    t = sch.get("type")
    if t is None and "properties" in sch:
        t = "object"
    if isinstance(t, list):
        if not t:
            raise ValueError("type list is empty")
        return ("alt", [_schema_ast(dict(sch, type=x), root, stack) for x in t])
    if t == "string":
        check({"type", "minLength", "maxLength"})
        lo, hi = sch.get("minLength", 0), sch.get("maxLength")
        if not isinstance(lo, int) or lo < 0 or (hi is not None and (not isinstance(hi, int) or hi < lo)):
            raise ValueError("bad minLength / maxLength")
        return ("cat", [lit('"'), ("rep", _STRING_CHAR, lo, hi), lit('"')])
    if t == "integer":
        check({"type"})
        return _INTEGER
    if t == "number":
        check({"type"})
        return _NUMBER
    if t == "boolean":
        check({"type"})
        return ("alt", [lit("true"), lit("false")])
    if t == "null":
        check({"type"})
        return lit("null")
    if t == "array":
        check({"type", "items", "minItems", "maxItems"})
        if "items" not in sch:
            raise ValueError("array schema needs 'items'")
        item = _schema_ast(sch["items"], root, stack)
        lo, hi = sch.get("minItems", 0), sch.get("maxItems")
        if not isinstance(lo, int) or lo < 0 or (hi is not None and (not isinstance(hi, int) or hi < lo)):
            raise ValueError("bad minItems / maxItems")
        if hi == 0:
            return lit("[]")
        more = ("rep", ("cat", [lit(","), _SP, item]), max(lo - 1, 0), None if hi is None else hi - 1)
        body = ("cat", [item, more])
        if lo == 0:
            body = ("rep", body, 0, 1)
        return ("cat", [lit("["), body, lit("]")])
    if t == "object":
        check({"type", "properties", "required", "additionalProperties"})
        props = sch.get("properties") or {}
        if not isinstance(props, dict):
            raise ValueError("properties must be an object")
        if not isinstance(sch.get("additionalProperties", False), bool):
            raise ValueError("unsupported JSON schema keyword: schema-valued additionalProperties")
        missing = [k for k in sch.get("required") or [] if k not in props]
        if missing:
            raise ValueError(f"required properties {missing} are not declared")
        items = [lit("{")]
        for i, (name, sub) in enumerate(props.items()):
            if i:
                items += [lit(","), _SP]
            items += [_json_lit(name), lit(":"), _SP, _schema_ast(sub, root, stack)]
        items.append(lit("}"))
        return ("cat", items)
    raise ValueError(f"unsupported JSON schema type {t!r}")


def compile_json_schema(schema, max_states: Optional[int] = None) -> Grammar:
    """Every declared property is emitted, in declaration order, and nothing else."""
    if isinstance(schema, str):
        try:
            schema = json.loads(schema)
        except json.JSONDecodeError as e:
            raise ValueError(f"guided_json is not valid JSON: {e}") from None
    if not isinstance(schema, dict):
        raise ValueError("a JSON schema must be an object")
    try:
        ast = _schema_ast(schema, schema, ())
    except RecursionError:
        raise ValueError("JSON schema nests too deeply") from None
    return _compile_ast(ast, "json", json.dumps(schema, sort_keys=False), max_states)


# ---------------------------------------------------------------- cache
_CACHE: "OrderedDict[tuple, Grammar]" = OrderedDict()
_CACHE_LOCK = threading.Lock()
CACHE_SIZE = 128


def _canonical(kind: str, spec) -> str:
    if kind == "regex":
        if not isinstance(spec, str):
            raise ValueError("guided_regex must be a string")
        return spec
    if kind == "json" and isinstance(spec, str):
        return spec
    try:
        return json.dumps(spec, sort_keys=False, separators=(",", ":"))
    except (TypeError, ValueError):
        raise ValueError(f"guided {kind} specification is not JSON-serialisable") from None


def compile_grammar(kind: str, spec, max_states: Optional[int] = None) -> Grammar:
    """LRU-cached compile of ("choice" | "regex" | "json", spec)."""
    if kind not in ("choice", "regex", "json"):
        raise ValueError(f"unknown constraint kind {kind!r}")
    key = (kind, _canonical(kind, spec), _cap(max_states))
    with _CACHE_LOCK:
        g = _CACHE.get(key)
        if g is not None:
            _CACHE.move_to_end(key)
            return g
    g = {"choice": compile_choice, "regex": compile_regex, "json": compile_json_schema}[kind](spec, max_states)
    with _CACHE_LOCK:
        _CACHE[key] = g
        while len(_CACHE) > CACHE_SIZE:
            _CACHE.popitem(last=False)
    return g
