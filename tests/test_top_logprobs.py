"""Top-N alternative log-probabilities (`top_logprobs`): the CPU reference op against the kernel's
contract, the OpenAI request mapping, the CPU engine with async scheduling on and off, and the
HTTP surface. The oracle and the engine checks are shared with tests/test_top_logprobs_gpu.py."""
import asyncio
import json

import aiohttp
import numpy as np
import pytest
import torch
from aiohttp import web

from llmd_amd import ops
from llmd_amd.engine.config import EngineConfig
from llmd_amd.engine.engine import LLMEngine
from llmd_amd.engine.request import SamplingParams
from llmd_amd.ops import reference as ref
from llmd_amd.serving.api_server import build_server

NEG_INF = float("-inf")
NMAX = 20
LP_ATOL = 1e-3  # the bound tests/test_sampling_gpu.py holds the sampler's log-probability to


# ---------------------------------------------------------------- oracle
def oracle(x, n_per_row):
    """x: CPU rows in the tested dtype. ids from a stable descending sort of those values,
    log-probabilities from a float64 log-softmax; -inf entries are never reported."""
    B, V = x.shape
    vals, order = torch.sort(x, dim=-1, descending=True, stable=True)
    logp = torch.log_softmax(x.double(), -1)
    ids = torch.full((B, NMAX), -1, dtype=torch.int64)
    lp = torch.full((B, NMAX), NEG_INF, dtype=torch.float64)
    for b in range(B):
        m = min(int(n_per_row[b]), V, int((x[b] > NEG_INF).sum()))
        ids[b, :m] = order[b, :m]
        lp[b, :m] = logp[b, order[b, :m]]
    return ids, lp


def check_against_oracle(x_cpu, n_per_row, got_ids, got_lp):
    assert got_ids.dtype == torch.int32 and got_lp.dtype == torch.float32
    assert tuple(got_ids.shape) == tuple(got_lp.shape) == (x_cpu.shape[0], NMAX)
    ids, lp = oracle(x_cpu, n_per_row)
    got_ids, got_lp = got_ids.cpu().long(), got_lp.cpu().double()
    bad = (got_ids != ids).any(-1).nonzero().flatten().tolist()
    assert not bad, f"rows {bad[:8]}: got {got_ids[bad[0]].tolist()} want {ids[bad[0]].tolist()}"
    live = ids >= 0
    assert (got_lp[~live] == NEG_INF).all()
    err = (got_lp[live] - lp[live]).abs().max().item() if live.any() else 0.0
    print(f"top_logprobs {tuple(x_cpu.shape)} {x_cpu.dtype}: max |lp - float64| = {err:.3e}")
    assert err <= LP_ATOL, err


def tie_rows(V, dtype):
    """Thirty entries equal to 9.0 over a background below 7, at the places where an index-order
    tie rule can go wrong: both ends of the row, a 16-byte chunk edge, one thread's chunks, spread."""
    per = 8 if dtype == torch.bfloat16 else 4          # entries per 16-byte chunk
    g = torch.Generator().manual_seed(3)
    places = {
        "ends": [0, V - 1, V - 2] + list(range(100, 127)),
        "chunk_edge": [per * 50 - 1, per * 50] + list(range(per * 300 - 14, per * 300 + 14)),
        # the chunks one thread of a 256- or 1024-wide workgroup reads
        "same_thread": [per * (5 + 1024 * k) + j for k in range(15) for j in (1, 6 % per)],
        "spread": np.linspace(3, V - 4, 30).astype(int).tolist(),
    }
    rows = []
    for name, idx in places.items():
        assert len(set(idx)) == 30 and max(idx) < V, name
        row = (torch.rand(V, generator=g) * 12 - 6).to(dtype)  # in [-6, 6)
        row[idx] = 9.0
        rows.append(row)
    return torch.stack(rows), [sorted(i)[:NMAX] for i in places.values()]


# ---------------------------------------------------------------- reference op
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_reference_contract(dtype):
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(6, 5003, generator=g) * 3).to(dtype)
    n = torch.tensor([1, 5, 20, 0, 20, 7], dtype=torch.int32)
    ids, lp = ops.top_logprobs(x, n)  # CPU tensors dispatch to the reference
    check_against_oracle(x, n.tolist(), ids, lp)
    assert (ids[3] == -1).all() and (lp[3] == NEG_INF).all()
    assert ops.MAX_TOP_LOGPROBS == NMAX == ref.MAX_TOP_LOGPROBS


def test_reference_ties_and_masks():
    x, want = tie_rows(128259, torch.bfloat16)
    ids, lp = ref.top_logprobs(x, torch.full((4,), 20, dtype=torch.int32))
    assert ids.tolist() == want
    check_against_oracle(x, [20] * 4, ids, lp)
    m = torch.full((3, 16), NEG_INF)
    m[0, [1, 4, 15]] = torch.tensor([0.5, 2.0, 0.5])
    m[1] = torch.arange(16).float()
    ids, lp = ref.top_logprobs(m, torch.tensor([20, 20, 20], dtype=torch.int32))
    assert ids[0].tolist() == [4, 1, 15] + [-1] * 17 and (lp[0, 3:] == NEG_INF).all()
    assert ids[1].tolist() == list(range(15, -1, -1)) + [-1] * 4
    assert (ids[2] == -1).all() and (lp[2] == NEG_INF).all()   # a fully masked row reports nothing
    check_against_oracle(m[:2], [20, 20], ids[:2], lp[:2])


# ---------------------------------------------------------------- request mapping
def test_from_openai_mapping():
    f = SamplingParams.from_openai
    with pytest.raises(ValueError):
        f({"logprobs": True, "top_logprobs": 21})
    with pytest.raises(ValueError):
        f({"top_logprobs": 2})
    with pytest.raises(ValueError):
        f({"logprobs": False, "top_logprobs": 2})
    with pytest.raises(ValueError):
        f({"logprobs": 21})
    with pytest.raises(ValueError):
        SamplingParams(top_logprobs=-1)._validated()
    sp = f({"logprobs": 3})
    assert sp.top_logprobs == 3 and sp.logprobs == 3
    sp = f({"logprobs": True})
    assert sp.top_logprobs == 0 and sp.logprobs
    sp = f({"logprobs": True, "top_logprobs": 2})
    assert sp.top_logprobs == 2 and sp.logprobs == 1
    sp = f({"logprobs": True, "top_logprobs": 0})
    assert sp.top_logprobs == 0 and sp.logprobs == 1
    sp = f({})
    assert sp.top_logprobs == 0 and sp.logprobs is None
    assert f({"logprobs": 0}).top_logprobs == 0


# ---------------------------------------------------------------- engine
def run_engine(device, async_scheduling, asking, other, **kw):
    """Two prompts in flight, `asking` and `other` their sampling parameters."""
    cfg = EngineConfig.create("tiny-llama", device=device, max_num_seqs=4, max_model_len=256,
                              enable_prefix_caching=False, async_scheduling=async_scheduling, **kw)
    eng = LLMEngine(cfg)
    rng = np.random.default_rng(0)
    a = eng.add_request("asks", rng.integers(3, 500, size=20).tolist(), asking)
    b = eng.add_request("plain", rng.integers(3, 500, size=13).tolist(), other)
    outs = []
    while eng.has_unfinished():
        outs.extend(eng.step())
    eng.shutdown()
    return a, b, outs


def check_greedy_invariants(a, b, outs, n_top, n_tok):
    assert len(a.output_token_ids) == len(a.output_logprobs) == len(a.output_top_logprobs) == n_tok
    for tok, lp, top in zip(a.output_token_ids, a.output_logprobs, a.output_top_logprobs):
        assert len(top) == n_top
        lps = [l for _, l in top]
        assert all(x >= y for x, y in zip(lps, lps[1:])) and all(np.isfinite(lps))
        assert top[0][0] == tok and abs(top[0][1] - lp) <= LP_ATOL
        assert len({t for t, _ in top}) == n_top
    assert len(b.output_token_ids) == n_tok and b.output_top_logprobs == [None] * n_tok
    # step outputs: the list only for the request that asked
    got = [o.new_top_logprobs[0] for o in outs if o.request_id == "asks"]
    assert got == a.output_top_logprobs
    assert all(o.new_top_logprobs is None for o in outs if o.request_id == "plain")


CPU_KW = dict(block_size=16, num_gpu_blocks=64, max_num_batched_tokens=64, enforce_eager=True)


def test_engine_cpu_greedy_async_and_sync():
    runs = []
    for async_on in (True, False):
        a, b, outs = run_engine("cpu", async_on,
                                SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True, top_logprobs=5),
                                SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True), **CPU_KW)
        check_greedy_invariants(a, b, outs, 5, 6)
        runs.append((a.output_token_ids, [[t for t, _ in top] for top in a.output_top_logprobs],
                     b.output_token_ids))
    assert runs[0] == runs[1]


@pytest.mark.parametrize("async_on", [True, False])
@pytest.mark.parametrize("n_top", [5, 20])
def test_engine_cpu_sampled_topk(async_on, n_top):
    """The list is taken from the tensor the sampler saw, after the top-k mask: only finite
    entries. top_k = 5 keeps 5 entries plus whatever ties with the fifth (topk_topp_mask keeps
    them), so with 20 asked for the list ends where the finite entries end, and the sampled
    token is always one of them."""
    a, _, _ = run_engine("cpu", async_on,
                         SamplingParams(max_tokens=8, temperature=1.0, top_k=5, seed=7, ignore_eos=True,
                                        logprobs=1, top_logprobs=n_top),
                         SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True), **CPU_KW)
    assert len(a.output_top_logprobs) == 8
    for tok, lp, top in zip(a.output_token_ids, a.output_logprobs, a.output_top_logprobs):
        assert 1 <= len(top) <= n_top and all(np.isfinite(l) and t >= 0 for t, l in top)
        lps = [l for _, l in top]
        assert all(x >= y for x, y in zip(lps, lps[1:]))
        d = dict(top)
        if n_top == 20:
            assert tok in d and len(top) < 20   # the mask left fewer than 20, the sampled one among them
        if tok in d:
            assert d[tok] == lp


# ---------------------------------------------------------------- HTTP
def _cfg():
    return EngineConfig.create("tiny-llama", device="cpu", block_size=16, num_gpu_blocks=128,
                               max_num_batched_tokens=128, max_num_seqs=8, max_model_len=512, enforce_eager=True)


async def _serve(app):
    runner = web.AppRunner(app, access_log=None)
    await runner.setup()
    site = web.TCPSite(runner, "127.0.0.1", 0)
    await site.start()
    return runner, site._server.sockets[0].getsockname()[1]


def _sse(text):
    return [json.loads(l[5:]) for l in text.splitlines() if l.startswith("data:") and "[DONE]" not in l]


@pytest.fixture(scope="module")
def http():
    """One server, every request of the HTTP tests, answers by name."""
    async def main():
        srv = build_server(_cfg())
        r1, port = await _serve(srv.app())
        comp = f"http://127.0.0.1:{port}/v1/completions"
        chat = f"http://127.0.0.1:{port}/v1/chat/completions"
        msgs = [{"role": "user", "content": "hi"}]
        base = {"max_tokens": 5, "temperature": 0, "ignore_eos": True}
        out = {}
        try:
            async with aiohttp.ClientSession() as s:
                async def post(name, url, body, sse=False):
                    async with s.post(url, json=dict(base, **body)) as r:
                        out[name + "_status"] = r.status
                        out[name] = _sse(await r.text()) if sse else await r.json()
                await post("comp3", comp, {"prompt": [5, 6, 7], "logprobs": 3, "return_token_ids": True})
                await post("comp_plain", comp, {"prompt": [5, 6, 7]})
                await post("comp_stream", comp, {"prompt": [5, 6, 7], "logprobs": 2, "stream": True,
                                                 "stream_options": {"include_usage": True}}, sse=True)
                await post("chat2", chat, {"messages": msgs, "logprobs": True, "top_logprobs": 2,
                                           "return_token_ids": True})
                await post("chat_true", chat, {"messages": msgs, "logprobs": True})
                await post("chat_plain", chat, {"messages": msgs})
                await post("chat_stream", chat, {"messages": msgs, "logprobs": True, "top_logprobs": 2,
                                                 "stream": True, "stream_options": {"include_usage": True}},
                           sse=True)
                await post("chat_stream_plain", chat, {"messages": msgs, "stream": True}, sse=True)
                await post("chat21", chat, {"messages": msgs, "logprobs": True, "top_logprobs": 21})
                await post("chat_nolp", chat, {"messages": msgs, "top_logprobs": 2})
                await post("comp21", comp, {"prompt": [5], "logprobs": 21})
            out["tok"] = srv.tok
            return out
        finally:
            await r1.cleanup()
            srv.aeng.shutdown()

    return asyncio.run(main())


def test_http_completions_logprobs(http):
    ch = http["comp3"]["choices"][0]
    lp, toks = ch["logprobs"], ch["token_ids"]
    assert set(lp) == {"tokens", "token_logprobs", "top_logprobs", "text_offset"}
    strs = [http["tok"].decode([t]) for t in toks]
    assert lp["tokens"] == strs and len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == 5
    assert lp["text_offset"] == [sum(len(s) for s in strs[:i]) for i in range(5)]
    for s, l, top in zip(strs, lp["token_logprobs"], lp["top_logprobs"]):
        assert 1 <= len(top) <= 3 and all(np.isfinite(v) for v in top.values())
        assert top[s] == pytest.approx(l, abs=1e-6) and l == max(top.values())  # greedy: the sampled token leads


def test_http_chat_logprobs(http):
    ch = http["chat2"]["choices"][0]
    content = ch["logprobs"]["content"]
    assert len(content) == http["chat2"]["usage"]["completion_tokens"] == 5
    for t, e in zip(ch["token_ids"], content):
        assert set(e) == {"token", "logprob", "bytes", "top_logprobs"}
        s = http["tok"].decode([t])
        assert e["token"] == s and e["bytes"] == list(s.encode("utf-8"))
        assert len(e["top_logprobs"]) == 2
        for a in e["top_logprobs"]:
            assert set(a) == {"token", "logprob", "bytes"} and a["bytes"] == list(a["token"].encode("utf-8"))
        assert e["top_logprobs"][0]["token"] == s
        assert e["top_logprobs"][0]["logprob"] == pytest.approx(e["logprob"], abs=1e-6)
        assert e["top_logprobs"][0]["logprob"] >= e["top_logprobs"][1]["logprob"]
    only = http["chat_true"]["choices"][0]["logprobs"]["content"]
    assert len(only) == 5 and all(e["top_logprobs"] == [] and np.isfinite(e["logprob"]) for e in only)
    # the same greedy run: the same sampled-token numbers with and without alternatives
    assert [e["logprob"] for e in only] == pytest.approx([e["logprob"] for e in content], abs=1e-6)


def test_http_stream_logprobs(http):
    chunks = http["chat_stream"]
    n = chunks[-1]["usage"]["completion_tokens"]
    ents = [e for c in chunks for ch in c["choices"] for e in (ch.get("logprobs") or {}).get("content", [])]
    assert n == 5 and len(ents) == n and all(len(e["top_logprobs"]) == 2 for e in ents)
    ref_ents = http["chat2"]["choices"][0]["logprobs"]["content"]
    assert [e["token"] for e in ents] == [e["token"] for e in ref_ents]
    chunks = http["comp_stream"]
    lps = [ch["logprobs"] for c in chunks for ch in c["choices"] if ch.get("logprobs")]
    toks = [t for l in lps for t in l["tokens"]]
    assert len(toks) == chunks[-1]["usage"]["completion_tokens"] == 5
    assert [o for l in lps for o in l["text_offset"]] == [sum(len(s) for s in toks[:i]) for i in range(5)]
    assert all(1 <= len(d) <= 2 for l in lps for d in l["top_logprobs"])


def test_http_validation_and_unchanged_without_logprobs(http):
    assert http["chat21_status"] == 400 and http["chat_nolp_status"] == 400 and http["comp21_status"] == 400
    # not requested: the keys every response had before this feature, and nothing else
    assert set(http["comp_plain"]["choices"][0]) == {"index", "finish_reason", "text"}
    assert set(http["chat_plain"]["choices"][0]) == {"index", "finish_reason", "message"}
    assert http["chat_plain"]["choices"][0].get("logprobs") is None
    assert set(http["chat_plain"]["choices"][0]["message"]) == {"role", "content"}
    for c in http["chat_stream_plain"]:
        assert all(set(ch) == {"index", "finish_reason", "delta"} for ch in c["choices"])


def test_http_stream_interval_groups_logprobs():
    """--stream-interval 2: a chunk covers several tokens and carries the entries of exactly
    those; over the stream they still number completion_tokens, in order."""
    from llmd_amd.serving.api_server import ServingOptions

    async def main():
        srv = build_server(_cfg(), opts=ServingOptions(stream_interval=2))
        r1, port = await _serve(srv.app())
        try:
            async with aiohttp.ClientSession() as s:
                async with s.post(f"http://127.0.0.1:{port}/v1/chat/completions",
                                  json={"messages": [{"role": "user", "content": "hi"}], "max_tokens": 5,
                                        "temperature": 0, "ignore_eos": True, "logprobs": True, "top_logprobs": 3,
                                        "stream": True, "stream_options": {"include_usage": True}}) as r:
                    return _sse(await r.text())
        finally:
            await r1.cleanup()
            srv.aeng.shutdown()

    chunks = asyncio.run(main())
    per_chunk = [len(ch["logprobs"]["content"]) for c in chunks for ch in c["choices"] if ch.get("logprobs")]
    assert per_chunk == [2, 2, 1] and chunks[-1]["usage"]["completion_tokens"] == 5
    ents = [e for c in chunks for ch in c["choices"] for e in (ch.get("logprobs") or {}).get("content", [])]
    assert all(len(e["top_logprobs"]) == 3 and e["top_logprobs"][0]["token"] == e["token"] for e in ents)
