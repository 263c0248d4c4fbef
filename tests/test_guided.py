"""Structured outputs on the CPU: the grammar compiler (llmd_amd/guided) against ``re`` and a
hand-written JSON validator, the token byte tables, the oracle of ``ops.guided_mask``, the
engine (tiny-llama, ByteTokenizer: byte tokens at ids 3..258, EOS 2) and the API server.
The kernel itself is checked in tests/test_guided_gpu.py."""
import asyncio
import json
import re

import aiohttp
import numpy as np
import pytest
import torch
from aiohttp import web

from llmd_amd import guided, ops
from llmd_amd.engine.config import EngineConfig
from llmd_amd.engine.engine import LLMEngine
from llmd_amd.engine.request import SamplingParams
from llmd_amd.guided import TokenTable, compile_choice, compile_grammar, compile_json_schema, compile_regex
from llmd_amd.ops import reference as ref
from llmd_amd.serving.api_server import build_server
from llmd_amd.serving.tokenizer import ByteTokenizer, HFTokenizer

EOS = 2


# ---------------------------------------------------------------- helpers (shared with the GPU tests)
def dist_to_accept(g):
    """Per state, the number of bytes of the shortest way to an accepting state."""
    S = g.num_states
    d = np.full(S, 1 << 30, dtype=np.int64)
    d[np.flatnonzero(g.accept)] = 0
    t = g.trans.astype(np.int64)
    for _ in range(S):
        nd = np.minimum(d, d[t].min(axis=1) + 1)
        nd[0] = 1 << 30
        if (nd == d).all():
            break
        d = nd
    return d


def random_walk(g, rng, max_len=24, stop_p=0.3, d=None):
    """Bytes of a random accepted string: random live transitions, then - past max_len - the
    shortest way to an accepting state."""
    d = dist_to_accept(g) if d is None else d
    s, out = 1, bytearray()
    while True:
        nxt = np.flatnonzero(g.trans[s])
        if g.accept[s] and (nxt.size == 0 or rng.random() < stop_p or len(out) >= max_len):
            return bytes(out)
        if len(out) >= max_len:
            nxt = nxt[d[g.trans[s, nxt]] == d[g.trans[s, nxt]].min()]
        b = int(rng.choice(nxt))
        out.append(b)
        s = int(g.trans[s, b])


ALPHABET = list("ab09 _-.@\n\tZ") + ["é", "日", "😀", "\x00", "\x7f", "߿", "￿"]


def mutate(s: str, rng) -> str:
    k = int(rng.integers(0, 3))
    i = int(rng.integers(0, len(s) + 1))
    c = ALPHABET[int(rng.integers(0, len(ALPHABET)))]
    if k == 0 or not s:
        return s[:i] + c + s[i:]
    i = min(i, len(s) - 1)
    return s[:i] + s[i + 1:] if k == 1 else s[:i] + c + s[i + 1:]


# ---------------------------------------------------------------- regex against re
PATTERNS = [
    r"abc", r"a|bc|def", r"(ab|cd)*e?", r"[0-9]{3}-[a-f]+", r"\d+\.\d{2}", r"\w+@\w+\.(com|org)",
    r"\s*x\s+y", r"\D\W\S", r".", r".*", r"a.+b", r"[^a-c]x", r"[^\d\s]+", r"[\w.-]{2,5}", r"(?:ab)+c",
    r"^ab+c$", r"a{2}", r"a{2,}", r"a{1,3}b{0,2}", r"\(\[\{\}\]\)\.\*\+\?\|\\\^\$", r"\n\t\r", r"[a-zA-Z_][a-zA-Z0-9_]*",
    r"é+|日本", r"[à-ÿ]+", r"[^é]", r"[Ѐ-ӿ]{1,2}z", r"[😀-😏]|[\x41-\x43]", r"(a|b)?(c|d)*(e|f)+",
    r"-?(0|[1-9][0-9]*)", r"[]a]+", r"[a\-z]+", r"x[^\n]*", r"(\d{1,3}\.){3}\d{1,3}",
]


@pytest.mark.parametrize("pat", PATTERNS)
def test_regex_matches_re(pat):
    """Accept / reject equals re.fullmatch(p, s, re.ASCII) on random walks of the DFA and on
    their mutations (with non-ASCII characters); no string is left out of the comparison."""
    g = compile_regex(pat)
    rx = re.compile(pat, re.ASCII)
    rng = np.random.default_rng(len(pat) * 7919 + sum(map(ord, pat)))
    d = dist_to_accept(g)
    n_pos = n_neg = 0
    for _ in range(60):
        w = random_walk(g, rng, max_len=12, d=d)
        s = w.decode("utf-8")  # every accepted byte string is well-formed UTF-8
        assert rx.fullmatch(s) is not None, (pat, s)
        n_pos += 1
        m = s
        for _ in range(3):
            m = mutate(m, rng)
            want = rx.fullmatch(m) is not None
            assert g.accepts(m.encode("utf-8")) == want, (pat, m)
            n_neg += not want
    assert n_pos == 60 and n_neg > 0


def test_regex_dfa_shape():
    g = compile_regex(r"[0-9]{3}-[a-f]+")
    assert g.trans.dtype == np.uint16 and g.trans.shape == (g.num_states, 256)
    assert g.accept.dtype == np.uint8 and g.accept.shape == (g.num_states,)
    assert not g.trans[0].any() and not g.accept[0]
    # trimmed: every live state is accepting or has a continuation, and reaches an accepting state
    assert all(g.accept[s] or g.trans[s].any() for s in range(1, g.num_states))
    assert (dist_to_accept(g)[1:] < 1 << 30).all()


ILL_FORMED = [b"\x80", b"\xc3", b"\xc0\x80", b"\xc1\xbf", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80",
              b"\xf8\x88\x80\x80\x80", b"\xe6\x97", b"a\xffb", b"\xf0\x80\x80\x80", b"\xc3\x28"]


@pytest.mark.parametrize("pat", [r".*", r"[^a]*", r"\D*", r"\W+", r"\S*", r"(.|\n)*", r"[^\x00]{0,4}"])
def test_no_dfa_accepts_ill_formed_utf8(pat):
    g = compile_regex(pat)
    for bad in ILL_FORMED:
        assert not g.accepts(bad), (pat, bad)
        assert not g.accepts(b"ok" + bad) and not g.accepts(bad + b"ok")
    assert g.accepts("é日😀".encode()) and g.accepts("߿￿\U0010ffff".encode())


def test_dot_and_negated_classes_by_hand():
    """Where the subset is defined without reference to re: one scalar value per '.', no newline."""
    g = compile_regex(r".")
    assert g.accepts(b"a") and g.accepts("😀".encode()) and not g.accepts(b"\n") and not g.accepts(b"ab")
    assert not g.accepts("é".encode()[:1])
    g = compile_regex(r"[^a]")
    assert g.accepts(b"\n") and g.accepts("日".encode()) and not g.accepts(b"a")


@pytest.mark.parametrize("pat", [r"(a)\1", r"(?=a)b", r"(?!a)b", r"(?<=a)b", r"a*?", r"a+?", r"a??", r"a{1,2}?", r"a*+",
                                 r"(?i)a", r"(?P<n>a)", r"\bword", r"a^b", r"a$b", r"(ab", r"ab)", r"[a-", r"a{2,1}",
                                 r"*a", r"[z-a]", "a\\"])
def test_unsupported_regex_raises(pat):
    with pytest.raises(ValueError):
        compile_regex(pat)


def test_state_cap():
    with pytest.raises(ValueError, match="states"):
        compile_regex(r"[a-z]{9000}")
    with pytest.raises(ValueError, match="states"):
        compile_regex(r"[a-z]{40}", max_states=32)
    with pytest.raises(ValueError, match="states"):
        compile_choice(["abcdefghij"], max_states=8)
    assert compile_regex(r"[a-z]{40}", max_states=64).num_states == 42
    # the cap can never exceed what uint16 holds
    with pytest.raises(ValueError):
        compile_regex(r"[a-z]{70000}", max_states=1 << 20)


def test_choice_trie():
    ch = ["yes", "no", "not sure", "née"]
    g = compile_choice(ch)
    for c in ch:
        assert g.accepts(c.encode())
    for bad in ["", "ye", "yess", "n", "not", "not  sure", "NO"]:
        assert not g.accepts(bad.encode())
    assert g.is_accepting(g.advance(1, b"no")) and g.advance(g.advance(1, b"no"), b"t") != 0
    for bad in ([], [""], ["a", 3], "abc", None):
        with pytest.raises(ValueError):
            compile_choice(bad)


def test_compile_cache():
    a = compile_grammar("regex", r"cache-me-[0-9]+")
    assert compile_grammar("regex", r"cache-me-[0-9]+") is a
    assert compile_grammar("choice", ["x", "y"]) is compile_grammar("choice", ["x", "y"])
    assert compile_grammar("choice", ["y", "x"]) is not compile_grammar("choice", ["x", "y"])
    s = {"type": "object", "properties": {"a": {"type": "integer"}}}
    assert compile_grammar("json", s) is compile_grammar("json", json.loads(json.dumps(s)))


# ---------------------------------------------------------------- JSON schema
SCHEMAS = {
    "flat": {"type": "object", "title": "T", "description": "d",
             "properties": {"name": {"type": "string", "minLength": 1, "maxLength": 6}, "age": {"type": "integer"},
                            "score": {"type": "number"}, "ok": {"type": "boolean"}, "none": {"type": "null"}},
             "required": ["name", "age"], "additionalProperties": False},
    "nested": {"type": "object", "properties": {
        "id": {"type": "integer"},
        "pos": {"type": "object", "properties": {"x": {"type": "number"}, "y": {"type": "number"},
                                                 "tag": {"type": "object", "properties": {"s": {"type": "string"}}}}}}},
    "array": {"type": "array", "items": {"type": "integer"}, "minItems": 2, "maxItems": 4},
    "array0": {"type": "object", "properties": {"xs": {"type": "array", "items": {"type": "boolean"}, "maxItems": 2},
                                                "ys": {"type": "array", "items": {"type": "string", "maxLength": 2}}}},
    "enum": {"enum": ["red", "gr\"een", 3, 2.5, None, True, {"a": [1, 2]}]},
    "const": {"type": "object", "properties": {"v": {"const": "é日"}}},
    "anyOf": {"anyOf": [{"type": "integer"}, {"type": "string", "maxLength": 3},
                        {"type": "object", "properties": {"k": {"type": ["boolean", "null"]}}}]},
    "oneOf": {"oneOf": [{"type": "null"}, {"type": "array", "items": {"enum": ["a", "b"]}, "minItems": 1}]},
    "ref": {"type": "object", "$defs": {"pt": {"type": "object", "properties": {"x": {"type": "integer"},
                                                                                   "y": {"type": "integer"}}}},
            "definitions": {"nm": {"type": "string", "maxLength": 4}},
            "properties": {"a": {"$ref": "#/$defs/pt"}, "b": {"$ref": "#/$defs/pt"},
                           "n": {"$ref": "#/definitions/nm"}}},
}


def validate(v, sch, root):
    """Validator of the supported subset (every declared property present, in order, nothing else)."""
    if "$ref" in sch:
        _, table, name = sch["$ref"].split("/")
        return validate(v, root[table][name], root)
    if "enum" in sch:
        return any(type(v) is type(e) and v == e for e in sch["enum"])
    if "const" in sch:
        return v == sch["const"]
    for k in ("anyOf", "oneOf"):
        if k in sch:
            return any(validate(v, s, root) for s in sch[k])
    t = sch.get("type", "object" if "properties" in sch else None)
    if isinstance(t, list):
        return any(validate(v, dict(sch, type=x), root) for x in t)
    if t == "string":
        return isinstance(v, str) and sch.get("minLength", 0) <= len(v) <= sch.get("maxLength", 1 << 30)
    if t == "integer":
        return isinstance(v, int) and not isinstance(v, bool)
    if t == "number":
        return isinstance(v, (int, float)) and not isinstance(v, bool)
    if t == "boolean":
        return isinstance(v, bool)
    if t == "null":
        return v is None
    if t == "array":
        return (isinstance(v, list) and sch.get("minItems", 0) <= len(v) <= sch.get("maxItems", 1 << 30)
                and all(validate(x, sch["items"], root) for x in v))
    if t == "object":
        props = sch.get("properties", {})
        return (isinstance(v, dict) and list(v) == list(props)
                and all(validate(v[k], s, root) for k, s in props.items()))
    raise AssertionError(sch)


@pytest.mark.parametrize("name", list(SCHEMAS))
def test_json_schema_walks_parse_and_validate(name):
    sch = SCHEMAS[name]
    g = compile_json_schema(sch)
    rng = np.random.default_rng(len(name))
    d = dist_to_accept(g)
    seen = set()
    for _ in range(40):
        w = random_walk(g, rng, max_len=60, stop_p=1.0, d=d)
        v = json.loads(w.decode("utf-8"))
        assert validate(v, sch, sch), (name, w)
        seen.add(w)
    assert len(seen) > 1
    # the whitespace policy: nothing but at most one space after ':' and ','
    assert not g.accepts(b" " + next(iter(seen))) and not g.accepts(next(iter(seen)) + b"\n")


def test_json_schema_by_hand():
    g = compile_json_schema(SCHEMAS["flat"])
    assert g.accepts(b'{"name":"bo","age":3,"score":-1.5e3,"ok":true,"none":null}')
    assert g.accepts(b'{"name": "b\\"o", "age": -7, "score": 0, "ok": false, "none": null}')
    assert g.accepts('{"name":"é日","age":0,"score":1,"ok":true,"none":null}'.encode())
    for bad in [b'{"name":"","age":3,"score":1,"ok":true,"none":null}',          # minLength
                b'{"name":"toolong7","age":3,"score":1,"ok":true,"none":null}',  # maxLength
                b'{"name":"a","age":03,"score":1,"ok":true,"none":null}',        # leading zero
                b'{"name":"a","age":3.0,"score":1,"ok":true,"none":null}',       # integer
                b'{"age":3,"name":"a","score":1,"ok":true,"none":null}',         # order
                b'{"name":"a","age":3,"score":1,"ok":true}',                     # missing
                b'{"name":"a","age":3,"score":1,"ok":true,"none":null,"x":1}',   # undeclared
                b'{"name":"a\nb","age":3,"score":1,"ok":true,"none":null}',      # control character
                b'{"name":"a\\x","age":3,"score":1,"ok":true,"none":null}',      # bad escape
                b'{"name":"a"b","age":3,"score":1,"ok":true,"none":null}',       # unescaped quote
                b'{"name":"a","age":3,  "score":1,"ok":true,"none":null}']:      # two spaces
        assert not g.accepts(bad), bad
    assert compile_json_schema(json.dumps(SCHEMAS["array"])).accepts(b"[1, 2,3]")
    assert not compile_json_schema(SCHEMAS["array"]).accepts(b"[1]")


@pytest.mark.parametrize("sch", [
    {"type": "string", "pattern": "a+"}, {"type": "string", "format": "date"}, {"allOf": [{"type": "integer"}]},
    {"not": {"type": "integer"}}, {"if": {"type": "integer"}, "then": {"type": "integer"}},
    {"type": "object", "patternProperties": {"a": {"type": "integer"}}}, {"type": "integer", "minimum": 3},
    {"type": "array", "items": {"type": "integer"}, "uniqueItems": True}, {"type": "array"},
    {"type": "object", "properties": {"a": {"type": "integer"}}, "additionalProperties": {"type": "integer"}},
    {"type": "object", "properties": {"a": {"type": "integer"}}, "required": ["b"]},
    {"$defs": {"n": {"type": "object", "properties": {"next": {"$ref": "#/$defs/n"}}}}, "$ref": "#/$defs/n"},
    {"$ref": "#/$defs/missing"}, {"$ref": "http://example.com/s.json"}, {"type": "frob"}, {}, {"title": "only"},
    {"enum": []}, {"type": "string", "minLength": 3, "maxLength": 2}, "not json", [1, 2],
])
def test_unsupported_schema_raises(sch):
    with pytest.raises(ValueError):
        compile_json_schema(sch)


# ---------------------------------------------------------------- token tables
def test_byte_tokenizer_table():
    tok = ByteTokenizer(512)
    data, off = tok.token_bytes(512)
    assert data.dtype == np.uint8 and off.dtype == np.int32 and off.shape == (513,)
    t = TokenTable(data, off).check_guidable()
    assert [t.token(i) for i in (0, 1, 2, 3, 68, 258, 259, 511)] == [b"", b"", b"", b"\x00", b"A", b"\xff", b"", b""]
    ids = tok.encode("héllo 日本")
    assert b"".join(t.token(i) for i in ids) == "héllo 日本".encode()
    # a table that lacks a byte is refused for guided requests, with the reason
    short = TokenTable(data[:-1], np.minimum(off, 255))
    with pytest.raises(ValueError, match="single-byte"):
        short.check_guidable()
    with pytest.raises(ValueError):
        TokenTable(data, off[::-1].copy())


def test_hf_bytelevel_bpe_table(tmp_path):
    """A ByteLevel BPE tokenizer trained here from an in-memory corpus: the token bytes are the
    bytes of decode(), token by token and over whole encodings."""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, trainers

    tk = Tokenizer(models.BPE())
    tk.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tk.decoder = decoders.ByteLevel()
    corpus = ["the quick brown fox jumps over the lazy dog", "héllo wörld, naïve café", "日本語のテキスト 😀 emoji",
              '{"name": "value", "n": 123}', "tabs\tand\nnewlines"] * 20
    tk.train_from_iterator(corpus, trainers.BpeTrainer(vocab_size=400, special_tokens=["<s>", "</s>"],
                                                       initial_alphabet=pre_tokenizers.ByteLevel.alphabet()))
    path = tmp_path / "tokenizer.json"
    tk.save(str(path))
    tok = HFTokenizer(str(path))
    data, off = tok.token_bytes(tok.vocab_size + 7)  # the model's vocabulary may be padded
    t = TokenTable(data, off).check_guidable()
    assert t.vocab_size == tok.vocab_size + 7
    assert t.token(0) == b"" and t.token(1) == b"" and t.token(tok.vocab_size + 3) == b""  # special / padding
    assert max(len(t.token(i)) for i in range(t.vocab_size)) > 2                            # merges were learnt
    for text in corpus[:5] + ["unseen: ¿qué? 你好 \x00\x7f"]:
        ids = tok.encode(text)
        assert b"".join(t.token(i) for i in ids) == tok.decode(ids).encode("utf-8") == text.encode("utf-8")


def test_hf_byte_fallback_and_refusal(tmp_path):
    from tokenizers import Tokenizer, decoders, models

    vocab = {"<unk>": 0, "▁hi": 1, "▁": 2, "a": 3}
    vocab.update({f"<0x{b:02X}>": 4 + b for b in range(256)})
    tk = Tokenizer(models.BPE(vocab=vocab, merges=[], unk_token="<unk>", byte_fallback=True))
    tk.decoder = decoders.Sequence([decoders.Replace("▁", " "), decoders.ByteFallback(), decoders.Fuse()])
    tk.add_special_tokens(["<unk>"])
    tk.save(str(tmp_path / "tokenizer.json"))
    t = TokenTable(*HFTokenizer(str(tmp_path / "tokenizer.json")).token_bytes()).check_guidable()
    assert [t.token(i) for i in (0, 1, 2, 3, 4 + 0xE6)] == [b"", b" hi", b" ", b"a", b"\xe6"]
    tk.decoder = decoders.WordPiece()
    tk.save(str(tmp_path / "wp.json"))
    with pytest.raises(ValueError, match="decoder"):
        HFTokenizer(str(tmp_path / "wp.json")).token_bytes()


# ---------------------------------------------------------------- reference op
def synthetic_table(V, rng, eos=(), alphabet=None, long_tokens=3):
    """Token table with lengths 0, 1, 2..48 and a few tokens of 128 bytes, over `alphabet` bytes."""
    alphabet = np.arange(256, dtype=np.uint8) if alphabet is None else np.frombuffer(alphabet, dtype=np.uint8)
    lens = rng.integers(2, 49, size=V)
    kind = rng.random(V)
    lens[kind < 0.55] = 1
    lens[kind < 0.05] = 0
    lens[rng.choice(V, size=long_tokens, replace=False)] = 128
    for e in eos:
        lens[e] = 0
    off = np.zeros(V + 1, dtype=np.int32)
    np.cumsum(lens, out=off[1:])
    data = alphabet[rng.integers(0, alphabet.size, size=int(off[-1]))]
    return data, off


def test_reference_guided_mask_matches_python_loop():
    rng = np.random.default_rng(5)
    V, eos = 777, [2, 500]
    g1, g2 = compile_regex(r"[0-9]{3}-[a-f]+"), compile_choice(["alpha", "alps", "beta", "al"])
    data, off = synthetic_table(V, rng, eos, alphabet=b"0123456789-abcdeflpsht")
    cap = 64
    trans, accept = np.zeros((cap, 256), dtype=np.uint16), np.zeros(cap, dtype=np.uint8)
    o1, o2 = 3, 3 + g1.num_states + 5
    for o, g in ((o1, g1), (o2, g2)):
        trans[o:o + g.num_states], accept[o:o + g.num_states] = g.trans, g.accept
    rows = [(o1, g1, 1), (o1, g1, g1.advance(1, b"12")), (o1, g1, g1.advance(1, b"123-a")), (None, None, -1),
            (o2, g2, 1), (o2, g2, g2.advance(1, b"al")), (o2, g2, g2.advance(1, b"beta"))]
    x = torch.from_numpy(rng.normal(size=(len(rows), V)).astype(np.float32))
    want = x.clone()
    for r, (o, g, s) in enumerate(rows):
        if s < 0:
            continue
        for t in range(V):
            tb = data[off[t]:off[t + 1]].tobytes()
            keep = bool(g.accept[s]) if t in eos else (len(tb) > 0 and g.advance(s, tb) != 0)
            if not keep:
                want[r, t] = float("-inf")
    got = ref.guided_mask(x.clone(), trans, accept, [o or 0 for o, _, _ in rows],
                          [g.num_states if g else 0 for _, g, _ in rows], [s for _, _, s in rows], data, off, eos)
    assert torch.equal(got, want)
    assert torch.equal(got[3], x[3]) and torch.isinf(got[6]).sum() == V - 2  # terminal state: only the EOS ids
    assert 0 < torch.isinf(got[0]).sum() < V
    # the op wrapper validates the per-row values against the arena before anything runs
    tt, ta = torch.from_numpy(trans), torch.from_numpy(accept)
    args = (tt, ta, [o1], [g1.num_states], [1], torch.from_numpy(data), torch.from_numpy(off), eos)
    assert torch.equal(ops.guided_mask(x[:1].clone(), *args), want[:1])
    for bad in [dict(state=[g1.num_states]), dict(state=[-2]), dict(off=[cap - 2]), dict(off=[-1]), dict(n=[1]),
                dict(eos=[V])]:
        a = (tt, ta, bad.get("off", [o1]), bad.get("n", [g1.num_states]), bad.get("state", [1]), args[5], args[6],
             bad.get("eos", eos))
        with pytest.raises(ValueError):
            ops.guided_mask(x[:1].clone(), *a)


# ---------------------------------------------------------------- engine
TOK = ByteTokenizer(512)


def make_engine(async_scheduling=True, **kw):
    opts = dict(device="cpu", block_size=16, num_gpu_blocks=64, max_num_batched_tokens=64, max_num_seqs=8,
                max_model_len=256, enforce_eager=True, enable_prefix_caching=False, async_scheduling=async_scheduling)
    opts.update(kw)
    eng = LLMEngine(EngineConfig.create("tiny-llama", **opts))
    assert eng.cfg.model_config.vocab_size == 512 and eng.cfg.model_config.eos_ids == [EOS]
    eng.set_token_table(TokenTable(*TOK.token_bytes(512)))
    return eng


def run(eng, jobs):
    """jobs: (prompt ids, params); returns the finished requests and every step output."""
    reqs = [eng.add_request(f"r{i}", p, sp) for i, (p, sp) in enumerate(jobs)]
    outs = []
    while eng.has_unfinished():
        outs.extend(eng.step())
    assert eng.bm.num_free() == eng.bm.num_blocks
    return reqs, outs


def text_of(r):
    toks = r.output_token_ids
    return bytes(t - 3 for t in (toks[:-1] if toks and toks[-1] == EOS else toks))


def check_guided_output(r, g):
    """Finished by the grammar: the whole output matches and ends on EOS. Cut by max_tokens: a
    prefix that the DFA keeps alive."""
    assert all(3 <= t < 259 for t in r.output_token_ids[:-1])
    b = text_of(r)
    if r.finish_reason == "stop":
        assert r.output_token_ids[-1] == EOS and g.accepts(b), b
    else:
        assert r.finish_reason == "length" and EOS not in r.output_token_ids and g.advance(1, b) != 0, b
    assert r.guided_state == g.advance(1, b)


PROMPT = TOK.encode("Answer: ")
CHOICES = ["yes", "no", "maybe so", "née"]


def test_engine_guided_choice_greedy_and_sampled():
    g = compile_choice(CHOICES)
    eng = make_engine()
    jobs = [(PROMPT, SamplingParams(max_tokens=20, temperature=0.0, guided=g))]
    jobs += [(PROMPT, SamplingParams(max_tokens=20, temperature=1.0, seed=s, guided=g)) for s in range(6)]
    reqs, _ = run(eng, jobs)
    for r in reqs:
        assert r.finish_reason == "stop" and text_of(r).decode() in CHOICES
        check_guided_output(r, g)
    assert len({text_of(r) for r in reqs}) > 1
    assert eng.runner.guided_arena.slots[g.uid][2] == 0  # unpinned once its requests finished


def test_engine_guided_regex_with_length_cut():
    g = compile_regex(r"[0-9]{3}-[a-f]+")
    eng = make_engine()
    jobs = [(PROMPT, SamplingParams(max_tokens=mt, temperature=t, seed=7 + mt, guided=g))
            for mt in (2, 4, 5, 9, 14) for t in (0.0, 1.0)]
    reqs, _ = run(eng, jobs)
    for r in reqs:
        check_guided_output(r, g)
    assert any(r.finish_reason == "length" for r in reqs)
    g2 = compile_regex(r"(ab|cd){2}e?")
    reqs, _ = run(eng, [(PROMPT, SamplingParams(max_tokens=12, temperature=1.0, seed=s, guided=g2)) for s in range(4)])
    for r in reqs:
        check_guided_output(r, g2)
        assert r.finish_reason == "stop"


def test_engine_async_and_sync_agree_beside_free_requests():
    """Greedy tokens are the same with async scheduling on and off, and a guided request does
    not change what the unconstrained requests beside it generate."""
    g = compile_regex(r"[0-9]{3}-[a-f]{2,6}")
    gc = compile_choice(CHOICES)
    free = [(TOK.encode("free text one"), SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True)),
            (TOK.encode("another"), SamplingParams(max_tokens=7, temperature=0.0, ignore_eos=True))]
    guided_jobs = [(PROMPT, SamplingParams(max_tokens=16, temperature=0.0, guided=g)),
                   (PROMPT, SamplingParams(max_tokens=16, temperature=0.0, guided=gc))]
    runs = {}
    for mode in (True, False):
        reqs, _ = run(make_engine(mode), free[:1] + guided_jobs + free[1:])
        runs[mode] = [r.output_token_ids for r in reqs]
        check_guided_output(reqs[1], g)
        check_guided_output(reqs[2], gc)
        assert reqs[1].finish_reason == reqs[2].finish_reason == "stop"
    assert runs[True] == runs[False]
    alone, _ = run(make_engine(True), free)
    assert [r.output_token_ids for r in alone] == [runs[True][0], runs[True][3]]


def test_engine_guided_survives_preemption():
    g = compile_regex(r"[a-f0-9]{30,40}")
    eng = make_engine(num_gpu_blocks=7, max_num_batched_tokens=64)
    jobs = [(TOK.encode("p" * 20 + str(i)), SamplingParams(max_tokens=48, temperature=0.0, guided=g)) for i in range(3)]
    reqs, _ = run(eng, jobs)
    assert eng.sched.num_preemptions_total > 0 and any(r.num_preemptions for r in reqs)
    for r in reqs:
        check_guided_output(r, g)
        assert r.finish_reason == "stop"
    ref_reqs, _ = run(make_engine(), jobs)
    assert [r.output_token_ids for r in reqs] == [r.output_token_ids for r in ref_reqs]


def test_engine_top_logprobs_never_list_a_forbidden_token():
    g = compile_regex(r"[0-9]{2}(ab|cd)x?")
    tt = TokenTable(*TOK.token_bytes(512))
    reqs, _ = run(make_engine(), [(PROMPT, SamplingParams(max_tokens=12, temperature=1.0, seed=3, guided=g,
                                                          logprobs=1, top_logprobs=20))])
    r, s = reqs[0], 1
    check_guided_output(r, g)
    for tok, top in zip(r.output_token_ids, r.output_top_logprobs):
        ok = {t for t in range(512) if (g.accept[s] if t == EOS else tt.token(t) and g.advance(s, tt.token(t)))}
        assert top and {t for t, _ in top} <= ok and len(top) == min(20, len(ok))
        assert all(np.isfinite(lp) for _, lp in top)
        s = g.advance(s, tt.token(tok))


def test_engine_refuses_bad_combinations():
    g = compile_choice(["a"])
    eng = make_engine()
    with pytest.raises(ValueError, match="ignore_eos"):
        eng.add_request("x", PROMPT, SamplingParams(guided=g, ignore_eos=True))
    with pytest.raises(ValueError, match="ignore_eos"):
        SamplingParams.from_openai({"guided_choice": ["a"], "ignore_eos": True})
    small = make_engine(guided_arena_states=40)
    big = compile_regex(r"[a-z]{60}")
    with pytest.raises(ValueError, match="arena"):
        small.add_request("big", PROMPT, SamplingParams(guided=big))
    # grammars of running requests are never evicted; idle ones make room
    a, b = compile_regex(r"[a-z]{20}"), compile_regex(r"[0-9]{20}")
    small.add_request("a", PROMPT, SamplingParams(guided=a, max_tokens=30))
    with pytest.raises(ValueError, match="arena"):
        small.add_request("b", PROMPT, SamplingParams(guided=b))
    while small.has_unfinished():
        small.step()
    rb = small.add_request("b", PROMPT, SamplingParams(guided=b, max_tokens=30, temperature=0.0))
    while small.has_unfinished():
        small.step()
    check_guided_output(rb, b)
    assert a.uid not in small.runner.guided_arena.slots
    bare = LLMEngine(EngineConfig.create("tiny-llama", device="cpu", num_gpu_blocks=16, enforce_eager=True))
    with pytest.raises(ValueError, match="byte table"):
        bare.add_request("x", PROMPT, SamplingParams(guided=g))


@pytest.mark.parametrize("stop_on", ["stop_token", "eos"])
def test_penalized_request_that_stops_under_async_scheduling(stop_on):
    """A request that needs settled tokens (a repetition penalty) and stops on a stop token or on
    EOS: async scheduling used to free it in the early drain while it was still in the step
    just scheduled ('block_table: unknown sequence'). Same tokens as the sync engine, and the
    engine lives on."""
    prompt = TOK.encode("penalties and a stop")
    kw = dict(temperature=0.0, repetition_penalty=1.2)
    probe, _ = run(make_engine(False), [(prompt, SamplingParams(max_tokens=8, ignore_eos=True, **kw))])
    toks = probe[0].output_token_ids
    if stop_on == "stop_token":
        sp = dict(max_tokens=8, stop_token_ids=[toks[3]], **kw)
        want = toks[:toks.index(toks[3]) + 1]
    else:
        sp = dict(max_tokens=8, logit_bias={EOS: 100.0}, min_tokens=0, **kw)
        want = [EOS]
    got = {}
    for mode in (True, False):
        eng = make_engine(mode)
        other = (TOK.encode("a free neighbour"), SamplingParams(max_tokens=10, temperature=0.0, ignore_eos=True))
        reqs, _ = run(eng, [(prompt, SamplingParams(**sp)), other])
        assert reqs[0].finish_reason == "stop" and len(reqs[1].output_token_ids) == 10
        again, _ = run(eng, [(prompt, SamplingParams(**sp))])  # a live engine
        assert again[0].output_token_ids == reqs[0].output_token_ids
        got[mode] = [r.output_token_ids for r in reqs]
    assert got[True] == got[False] and got[True][0] == want


# ---------------------------------------------------------------- API
def _cfg():
    return EngineConfig.create("tiny-llama", device="cpu", block_size=16, num_gpu_blocks=128,
                               max_num_batched_tokens=128, max_num_seqs=8, max_model_len=512, enforce_eager=True)


async def _serve(app):
    runner = web.AppRunner(app, access_log=None)
    await runner.setup()
    site = web.TCPSite(runner, "127.0.0.1", 0)
    await site.start()
    return runner, site._server.sockets[0].getsockname()[1]


API_SCHEMA = {"type": "object", "properties": {"ok": {"type": "boolean"}, "tag": {"enum": ["a", "b"]},
                                               "s": {"type": "string", "maxLength": 3},
                                               "xs": {"type": "array", "items": {"type": "null"}, "maxItems": 2}}}
API_REGEX = r"[0-9]{3}-[a-f]{1,4}"
FIELDS = {
    "guided_choice": ({"guided_choice": CHOICES}, "choice"),
    "guided_regex": ({"guided_regex": API_REGEX}, "regex"),
    "guided_json": ({"guided_json": API_SCHEMA}, "json"),
    "guided_json_str": ({"guided_json": json.dumps(API_SCHEMA)}, "json"),
    "so_choice": ({"structured_outputs": {"choice": CHOICES}}, "choice"),
    "so_regex": ({"structured_outputs": {"regex": API_REGEX}}, "regex"),
    "so_json": ({"structured_outputs": {"json": API_SCHEMA}}, "json"),
    "response_format": ({"response_format": {"type": "json_schema",
                                             "json_schema": {"name": "x", "schema": API_SCHEMA}}}, "json"),
}
BAD = {
    "two": {"guided_choice": ["a"], "guided_regex": "a"},
    "two_rf": {"guided_regex": "a", "response_format": {"type": "json_schema", "json_schema": {"schema": API_SCHEMA}}},
    "two_so": {"structured_outputs": {"choice": ["a"], "regex": "a"}},
    "bad_regex": {"guided_regex": "(a"},
    "unsupported_regex": {"guided_regex": r"(a)\1"},
    "bad_choice": {"guided_choice": []},
    "unsupported_schema": {"guided_json": {"type": "string", "pattern": "a+"}},
    "bad_json": {"guided_json": "{not json"},
    "bad_rf": {"response_format": {"type": "json_schema"}},
    "over_cap": {"guided_regex": r"[a-z]{9000}"},
    "ignore_eos": {"guided_choice": ["a"], "ignore_eos": True},
    "so_unknown": {"structured_outputs": {"grammar": "root ::= 'a'"}},
}


def _check_api_text(kind, text, finish):
    assert finish == "stop", (kind, text)
    if kind == "choice":
        assert text in CHOICES
    elif kind == "regex":
        assert re.fullmatch(API_REGEX, text)
    else:
        assert validate(json.loads(text), API_SCHEMA, API_SCHEMA), text


def test_api_guided_fields():
    async def main():
        srv = build_server(_cfg())
        r1, port = await _serve(srv.app())
        urls = {False: f"http://127.0.0.1:{port}/v1/completions", True: f"http://127.0.0.1:{port}/v1/chat/completions"}
        out = {}
        try:
            async with aiohttp.ClientSession() as s:
                async def post(chat, extra, **kw):
                    body = dict({"max_tokens": 64, "temperature": 1.0, "seed": 11}, **extra, **kw)
                    body.update({"messages": [{"role": "user", "content": "hi"}]} if chat else {"prompt": "Answer: "})
                    async with s.post(urls[chat], json=body) as r:
                        if body.get("stream") and r.status == 200:
                            return r.status, [json.loads(l[5:]) for l in (await r.text()).splitlines()
                                              if l.startswith("data:") and "[DONE]" not in l]
                        return r.status, await r.json()
                for chat in (False, True):
                    for name, (extra, kind) in FIELDS.items():
                        out[chat, name] = await post(chat, extra)
                    for name, extra in BAD.items():
                        out[chat, "bad", name] = await post(chat, extra)
                    out[chat, "stream"] = await post(chat, FIELDS["guided_regex"][0], stream=True)
                    out[chat, "json_object"] = await post(chat, {"response_format": {"type": "json_object"}},
                                                          max_tokens=4)
                    out[chat, "text"] = await post(chat, {"response_format": {"type": "text"}}, max_tokens=4)
                out["n2"] = await post(False, FIELDS["guided_choice"][0], n=2)
                srv2 = build_server(_cfg())
                tb = ByteTokenizer(512)
                data, off = tb.token_bytes(512)
                srv2.tok = type("NoZeroByte", (), {"encode": tb.encode, "decode": tb.decode, "token_bytes":
                                                   staticmethod(lambda v=None: (data[1:], np.maximum(off - 1, 0)))})()
                r2, port2 = await _serve(srv2.app())
                try:
                    for _ in range(2):
                        async with s.post(f"http://127.0.0.1:{port2}/v1/completions",
                                          json={"prompt": "x", "guided_choice": ["a"]}) as r:
                            out["tokenizer"] = (r.status, await r.json())
                    async with s.post(f"http://127.0.0.1:{port2}/v1/completions",
                                      json={"prompt": "x", "max_tokens": 2}) as r:
                        out["tokenizer_free"] = r.status
                finally:
                    await r2.cleanup()
                    srv2.aeng.shutdown()
            return out
        finally:
            await r1.cleanup()
            srv.aeng.shutdown()

    out = asyncio.run(main())
    for chat in (False, True):
        for name, (_, kind) in FIELDS.items():
            status, body = out[chat, name]
            assert status == 200, (chat, name, body)
            ch = body["choices"][0]
            _check_api_text(kind, ch["message"]["content"] if chat else ch["text"], ch["finish_reason"])
        for name in BAD:
            status, body = out[chat, "bad", name]
            assert status == 400 and body["error"]["message"], (chat, name, body)
        assert "states" in out[chat, "bad", "over_cap"][1]["error"]["message"]
        assert "ignore_eos" in out[chat, "bad", "ignore_eos"][1]["error"]["message"]
        status, chunks = out[chat, "stream"]
        assert status == 200
        parts = [c["choices"][0] for c in chunks if c["choices"]]
        text = "".join((p["delta"].get("content") or "") if chat else p["text"] for p in parts)
        _check_api_text("regex", text, [p["finish_reason"] for p in parts if p["finish_reason"]][-1])
        assert out[chat, "json_object"][0] == 200 and out[chat, "text"][0] == 200  # accepted, not enforced
    status, body = out["n2"]
    assert status == 200 and [c["index"] for c in body["choices"]] == [0, 1]
    for c in body["choices"]:
        _check_api_text("choice", c["text"], c["finish_reason"])
    assert out["tokenizer"][0] == 400 and "single-byte" in out["tokenizer"][1]["error"]["message"]
    assert out["tokenizer_free"] == 200
