"""Speculative decoding on the CPU reference ops (tiny-llama): draft-and-verify reproduces plain
decoding token for token whatever the proposer says, the n-gram index (native and Python), the
scheduler / runner plumbing, the startup refusals and the HTTP surface."""
import argparse
import asyncio
import json

import aiohttp
import numpy as np
import pytest
import torch
from aiohttp import web

from llmd_amd import _rt_loader, ops
from llmd_amd.engine.config import EngineConfig, add_engine_args, engine_config_from_args
from llmd_amd.engine.engine import LLMEngine
from llmd_amd.engine.model_runner import _mix64
from llmd_amd.engine.request import Request, SamplingParams
from llmd_amd.engine.spec_decode import PyNgramIndex, SpeculativeConfig, make_ngram_index
from llmd_amd.ops import reference as ref

K = 4
SPEC = {"method": "ngram", "num_speculative_tokens": K, "prompt_lookup_max": 4, "prompt_lookup_min": 2}
# periodic prompts (a short pattern repeated) and one plain ramp
PROMPTS = [[3, 4, 5, 6] * 6, list(range(10, 40)), [7, 8, 9] * 5, [100, 101] * 9 + [100]]
# tiny-llama (seed 0) answers this one with a single repeated token: n-gram drafts are accepted
REPEATING = [7, 8, 9] * 5
MAXT = 24
VOCAB = 512


def make_engine(spec=None, **kw):
    opts = dict(device="cpu", block_size=16, num_gpu_blocks=128, max_num_batched_tokens=256, max_num_seqs=8,
                max_model_len=512, enforce_eager=True)
    opts.update(kw)
    return LLMEngine(EngineConfig.create("tiny-llama", speculative_config=spec, **opts))


def greedy(max_tokens=MAXT, **kw):
    return SamplingParams(max_tokens=max_tokens, temperature=0.0, ignore_eos=True, logprobs=1, **kw)


@pytest.fixture(scope="module")
def base():
    """The spec-off run every proposer is built from and compared with (computed once)."""
    eng = make_engine()
    assert eng.spec is None and eng.async_sched  # nothing configured: async scheduling stays on
    reqs = eng.generate(PROMPTS, greedy(64))
    return {tuple(r.prompt_token_ids): list(r.output_token_ids) for r in reqs}


def proposer(base, right=K):
    """Drafts whose first ``right`` tokens are the baseline's and whose remaining ones are wrong."""
    def propose(r, k):
        want = base[tuple(r.prompt_token_ids)]
        n = len(r.output_token_ids)
        d = want[n:n + k]
        return [t if j < right else (t + 1) % VOCAB for j, t in enumerate(d)]
    return propose


def expected(n_req, max_tokens, k, right):
    """(drafts, draft tokens, accepted, accepted per position) of n_req requests that never stop early."""
    drafts = dtok = acc = 0
    pos = [0] * k
    n = 1  # the prefill step samples the first token
    while n < max_tokens:
        kk = min(k, max_tokens - n - 1)
        if kk <= 0:
            n += 1
            continue
        a = min(right, kk)
        drafts, dtok, acc = drafts + 1, dtok + kk, acc + a
        for j in range(a):
            pos[j] += 1
        n += a + 1
    return drafts * n_req, dtok * n_req, acc * n_req, [p * n_req for p in pos]


def check_equal(reqs, base, max_tokens=MAXT, reason="length"):
    for r in reqs:
        want = base[tuple(r.prompt_token_ids)][:max_tokens]
        assert r.output_token_ids == want
        assert len(r.output_logprobs) == len(r.output_top_logprobs) == len(want)
        assert r.finish_reason == reason


# ---------------------------------------------------------------- acceptance
@pytest.mark.parametrize("right", [K, 0, 1, 2, 3])  # oracle, always wrong, right for j tokens then wrong
def test_injected_proposer_reproduces_baseline(base, right):
    eng = make_engine(SPEC)
    assert not eng.async_sched  # the proposer reads token values
    eng.spec.proposer = proposer(base, right)
    reqs = eng.generate(PROMPTS, greedy())
    check_equal(reqs, base)
    d, t, a, pos = expected(len(PROMPTS), MAXT, K, right)
    sp = eng.spec
    assert (sp.num_drafts, sp.num_draft_tokens, sp.num_accepted_tokens, sp.accepted_per_pos) == (d, t, a, pos)
    text = eng.metrics.render().decode()
    m = eng.cfg.served_name
    assert f'vllm:spec_decode_num_drafts_total{{model_name="{m}"}} {float(d)}' in text
    assert f'vllm:spec_decode_num_draft_tokens_total{{model_name="{m}"}} {float(t)}' in text
    if a:
        assert f'vllm:spec_decode_num_accepted_tokens_total{{model_name="{m}"}} {float(a)}' in text
        assert (f'vllm:spec_decode_num_accepted_tokens_per_pos_total{{model_name="{m}",position="0"}} '
                f'{float(pos[0])}') in text
    assert f'vllm:generation_tokens_total{{model_name="{m}"}} {float(MAXT * len(PROMPTS))}' in text


def test_logprobs_equal_baseline(base):
    eng0 = make_engine()
    want = eng0.generate(PROMPTS, greedy())
    eng = make_engine(SPEC)
    eng.spec.proposer = proposer(base, 2)
    got = eng.generate(PROMPTS, greedy())
    for g, w in zip(got, want):
        assert g.output_token_ids == w.output_token_ids
        np.testing.assert_allclose(g.output_logprobs, w.output_logprobs, atol=1e-4)


def test_step_outputs_carry_every_new_token(base):
    eng = make_engine(SPEC)
    eng.spec.proposer = proposer(base)
    r = eng.add_request("a", PROMPTS[1], greedy())
    toks, lps, sizes = [], [], []
    while eng.has_unfinished():
        for o in eng.step():
            assert len(o.new_token_ids) == len(o.new_logprobs)
            toks += o.new_token_ids
            lps += o.new_logprobs
            sizes.append(len(o.new_token_ids))
    assert toks == r.output_token_ids == base[tuple(PROMPTS[1])][:MAXT] and lps == r.output_logprobs
    assert max(sizes) == K + 1  # a fully accepted run and its bonus token in one step


def test_ngram_proposer_reproduces_baseline(base):
    eng = make_engine(SPEC)
    reqs = eng.generate(PROMPTS, greedy(64))
    check_equal(reqs, base, 64)
    assert eng.spec.num_drafts > 0
    assert not eng.spec.proposer.index  # dropped with their requests


def test_ngram_accepts_on_repeating_output(base):
    out = base[tuple(REPEATING)]
    assert len(set(out[:20])) == 1  # the baseline starts with a run of one token
    eng = make_engine(SPEC)
    reqs = eng.generate([REPEATING], greedy(64))
    check_equal(reqs, base, 64)
    assert eng.spec.num_accepted_tokens > 0 and eng.step_count < 64


@pytest.mark.parametrize("max_tokens", [1, 2, 3, 5, 6, 7, 9])
def test_max_tokens_inside_accepted_run(base, max_tokens):
    eng = make_engine(SPEC)
    eng.spec.proposer = proposer(base)
    check_equal(eng.generate(PROMPTS, greedy(max_tokens)), base, max_tokens)


def test_stop_token_and_min_tokens_inside_accepted_run(base):
    p = PROMPTS[1]
    out = base[tuple(p)]
    # a token that first appears in the middle of a run of K + 1 emitted tokens
    idx = next(i for i in range(2, MAXT) if out[i] not in out[:i] and (i - 1) % (K + 1) not in (0, K))
    stop = out[idx]
    for min_tokens in (0, idx + 2):
        sp = SamplingParams(max_tokens=MAXT, temperature=0.0, stop_token_ids=[stop], min_tokens=min_tokens)
        want = make_engine().generate([p], sp)[0]
        eng = make_engine(SPEC)
        eng.spec.proposer = proposer(base)
        got = eng.generate([p], sp)[0]
        assert got.output_token_ids == want.output_token_ids
        assert got.finish_reason == want.finish_reason and got.stop_reason == want.stop_reason
        if min_tokens == 0:
            assert got.output_token_ids == out[:idx + 1] and got.finish_reason == "stop"
        else:
            assert len(got.output_token_ids) >= min_tokens


def test_preemption(base):
    """Three requests in 12 blocks of 16 with 64 output tokens each cannot all stay resident."""
    prompts = PROMPTS[:3]
    for prop in (proposer(base), proposer(base, 1), None):
        eng = make_engine(SPEC, num_gpu_blocks=12)
        if prop is not None:
            eng.spec.proposer = prop
        reqs = eng.generate(prompts, greedy(64))
        assert eng.sched.num_preemptions_total > 0
        check_equal(reqs, base, 64)
        assert eng.bm.num_free() == 12


def test_ineligible_requests_get_no_drafts(base):
    from llmd_amd.guided import TokenTable, compile_regex
    from llmd_amd.serving.tokenizer import ByteTokenizer

    asked = set()
    inner = proposer(base)

    def prop(r, k):
        asked.add(r.request_id)
        return inner(r, k)

    jobs = {
        "plain": (PROMPTS[0], greedy()),
        "penalised": (PROMPTS[1], greedy(presence_penalty=0.5)),
        "guided": (PROMPTS[2], SamplingParams(max_tokens=MAXT, temperature=0.0, guided=compile_regex(r"[a-c]{30}"))),
        "top": (PROMPTS[3], greedy(top_logprobs=2)),
    }
    outs = {}
    for spec in (None, SPEC):
        eng = make_engine(spec)
        eng.set_token_table(TokenTable(*ByteTokenizer(512).token_bytes(512)))
        if spec:
            eng.spec.proposer = prop
        reqs = {n: eng.add_request(n, p, sp) for n, (p, sp) in jobs.items()}
        while eng.has_unfinished():
            eng.step()
        outs[bool(spec)] = {n: (r.output_token_ids, r.finish_reason) for n, r in reqs.items()}
        if spec:
            assert eng.spec.num_accepted_tokens > 0
            assert all(len(t) == 2 for t in reqs["top"].output_top_logprobs)
    assert asked == {"plain"}
    assert outs[True] == outs[False]


def test_prefix_cache_after_rejected_drafts(base):
    """Blocks are hashed over the real tokens, never over rejected drafts: a follow-up whose prompt
    is the first prompt plus its output hits the cache and continues as the baseline does."""
    p = PROMPTS[1]
    res, by = {}, {}
    for spec in (None, SPEC):
        eng = make_engine(spec)
        if spec:
            eng.spec.proposer = proposer(by, 0)  # always wrong, for both requests
        first = eng.generate([p], greedy(40))[0]
        follow = eng.generate([p + first.output_token_ids], greedy(8))[0]
        res[bool(spec)] = (first.output_token_ids, follow.output_token_ids, follow.num_cached_tokens)
        by = {tuple(first.prompt_token_ids): first.output_token_ids,
              tuple(follow.prompt_token_ids): follow.output_token_ids}
    assert eng.spec.num_draft_tokens > 0 and eng.spec.num_accepted_tokens == 0
    assert res[True] == res[False]
    assert res[True][2] >= 64  # 30 + 40 tokens: four full blocks of 16


def test_seeded_sampling_rows_get_the_seed_of_their_position():
    eng = make_engine(SPEC)
    r = Request("s", [5, 6, 7], SamplingParams(temperature=0.8, seed=1234, max_tokens=32))
    r.output_token_ids = [9, 9, 9]
    o = Request("o", [5, 6, 7], SamplingParams(temperature=0.8, seed=77, max_tokens=32))
    temps, seeds, *_ = eng.runner._sampling_tensors([o, r, r, r, o])
    assert seeds.tolist() == [_mix64(77 * 1000003), *(_mix64(1234 * 1000003 + 3 + j) for j in range(3)),
                              _mix64(77 * 1000003)]
    # and plain decoding at those output lengths asks for the same seeds
    for j in range(3):
        r.output_token_ids = [9] * (3 + j)
        assert eng.runner._sampling_tensors([r])[1][0] == seeds[1 + j]


def test_sampled_requests_speculate():
    """temperature > 0: a verify step still runs and the request finishes with max_tokens tokens (the
    CPU reference sampler draws a step's rows from one generator: only the distribution is kept)."""
    eng = make_engine(SPEC)
    r = eng.generate([REPEATING], SamplingParams(max_tokens=20, temperature=0.7, seed=3, ignore_eos=True))[0]
    assert len(r.output_token_ids) == 20 and r.finish_reason == "length"


def test_windowed_model_without_hybrid_pool(base):
    """gpt-oss shapes (sliding window 16 + sinks) are eligible with the hybrid KV manager off."""
    kw = dict(hybrid_kv_cache_manager=False)
    cfg = dict(device="cpu", block_size=16, num_gpu_blocks=128, max_num_batched_tokens=256, max_num_seqs=8,
               max_model_len=512, enforce_eager=True, **kw)
    prompts = [list(range(20, 60)), [11, 12, 13] * 9]
    want = LLMEngine(EngineConfig.create("tiny-gpt-oss", **cfg)).generate(prompts, greedy(20))
    by = {tuple(r.prompt_token_ids): r.output_token_ids for r in want}
    for right in (K, 1):
        eng = LLMEngine(EngineConfig.create("tiny-gpt-oss", speculative_config=SPEC, **cfg))
        eng.spec.proposer = proposer(by, right)
        got = eng.generate(prompts, greedy(20))
        assert [r.output_token_ids for r in got] == [r.output_token_ids for r in want]
        assert eng.spec.num_accepted_tokens > 0


# ---------------------------------------------------------------- scheduler
def test_scheduler_layout_and_budget(base):
    eng = make_engine(SPEC, max_num_batched_tokens=40)
    eng.spec.proposer = proposer(base)
    a = eng.add_request("a", PROMPTS[0], greedy())
    while not a.output_token_ids:
        eng.step()
    eng.add_request("b", PROMPTS[1], greedy())
    so = eng.sched.schedule()
    assert [s.req.request_id for s in so.verifies] == ["a"] and not so.decodes
    v = so.verifies[0]
    assert v.num_new_tokens == 1 + K and list(v.drafts) == base[tuple(PROMPTS[0])][1:1 + K] and v.samples
    assert so.num_tokens == 1 + K + so.prefills[0].num_new_tokens <= 40
    assert [s.req.request_id for s in so.all()] == ["a", "b"]
    rows, reqs = eng.runner._sample_rows(so)
    assert rows[:1 + K] == list(range(1 + K)) and all(r is a for r in reqs[:1 + K])
    ids, pos, *_ = eng.runner._prepare(so, eng.block_tables(so))
    n = a.num_tokens
    assert ids[:1 + K] == [a.output_token_ids[-1]] + list(v.drafts) and pos[:1 + K] == list(range(n - 1, n + K))


def test_drafts_dropped_before_preempting(base):
    """No room for the drafts' blocks: the request decodes plainly and nobody is preempted."""
    eng = make_engine(SPEC, num_gpu_blocks=2, max_model_len=64)
    eng.spec.proposer = proposer(base)
    p = PROMPTS[1]  # 30 tokens: two blocks of 16 hold 32
    r = eng.add_request("a", p, greedy(8))
    eng.step()
    so = eng.sched.schedule()  # position 30 fits, 30 + K does not
    assert not so.verifies and len(so.decodes) == 1 and not so.preempted and eng.spec.num_drafts == 0
    assert r.output_token_ids == base[tuple(p)][:1]


# ---------------------------------------------------------------- n-gram index
def _streams():
    rng = np.random.default_rng(0)
    for vocab, n in ((3, 400), (8, 600), (50, 300)):
        yield rng.integers(0, vocab, n).tolist()
    yield [1, 2, 3] * 40
    yield [5]
    yield []


@pytest.mark.parametrize("lo,hi", [(1, 1), (2, 4), (3, 3), (1, 6)])
def test_ngram_native_equals_python(lo, hi):
    native = _rt_loader.rt().NgramIndex
    for toks in _streams():
        a, b = native(lo, hi), PyNgramIndex(lo, hi)
        rng = np.random.default_rng(len(toks))
        i = 0
        while i <= len(toks):
            step = int(rng.integers(1, 6))
            a.append(toks[i:i + step])
            b.append(toks[i:i + step])
            i += step
            n = min(i, len(toks))
            assert len(a) == len(b) == n
            for k in (1, 3, 7):
                got = list(a.propose(k))
                assert got == b.propose(k) and len(got) <= k
                # incremental appends give what a rebuild over the same tokens gives
                c = native(lo, hi)
                c.append(toks[:n])
                assert list(c.propose(k)) == got
            assert list(a.propose(0)) == b.propose(0) == []


def test_ngram_semantics():
    ix = make_ngram_index(2, 3)
    ix.append([1, 2, 3, 4, 9, 2, 3, 5, 6, 7, 1, 2, 3])
    # the longest suffix n-gram seen before is (1, 2, 3) -> what followed it
    assert list(ix.propose(4)) == [4, 9, 2, 3] and list(ix.propose(1)) == [4]
    ix.append([8, 2, 3])  # (8, 2, 3) is new; (2, 3) most recently continued with 8
    assert list(ix.propose(2)) == [8, 2]
    ix.append([99])
    assert list(ix.propose(3)) == []
    with pytest.raises(ValueError):
        PyNgramIndex(3, 2)
    with pytest.raises(ValueError):
        make_ngram_index(0, 2)


# ---------------------------------------------------------------- op (CPU path)
def test_paged_verify_cpu_rows_are_decode_rows():
    torch.manual_seed(0)
    kc, vc = torch.randn(8, 2, 16, 64).bfloat16(), torch.randn(8, 2, 16, 64).bfloat16()
    bt = torch.tensor([[1, 2, 3], [4, 5, 0]], dtype=torch.int32)
    sl = torch.tensor([40, 20], dtype=torch.int32)
    qs, ql = torch.tensor([0, 3], dtype=torch.int32), torch.tensor([3, 2], dtype=torch.int32)
    q = torch.randn(5, 4 * 64).bfloat16()
    sinks = torch.randn(4)
    for window in (0, 8):
        o = ops.paged_verify(q, kc, vc, bt, sl, qs, ql, 4, 2, 64, 0.125, window, sinks)
        for row, b, L in [(0, 0, 38), (1, 0, 39), (2, 0, 40), (3, 1, 19), (4, 1, 20)]:
            d = ref.paged_decode(q[row:row + 1], kc, vc, bt[b:b + 1], torch.tensor([L]), 4, 2, 64, 0.125,
                                 window, sinks)
            assert torch.equal(d[0], o[row])
    with pytest.raises(ValueError):
        ops.paged_verify(q, kc, vc, bt, sl, qs, torch.tensor([9, 2], dtype=torch.int32), 4, 2, 64, 0.125)
    with pytest.raises(ValueError):
        ops.paged_verify(torch.randn(5, 34 * 64).bfloat16(), kc, vc, bt, sl, qs, ql, 34, 2, 64, 0.125)


# ---------------------------------------------------------------- configuration and refusals
def test_speculative_config_parsing():
    sc = SpeculativeConfig.from_dict(SPEC)
    assert (sc.num_speculative_tokens, sc.prompt_lookup_max, sc.prompt_lookup_min) == (4, 4, 2)
    assert SpeculativeConfig.from_dict(None) is None
    sc = SpeculativeConfig.from_dict({"method": "ngram", "num_speculative_tokens": 7, "prompt_lookup_max": 5})
    assert (sc.prompt_lookup_max, sc.prompt_lookup_min) == (5, 5)
    for bad in ({"method": "eagle", "num_speculative_tokens": 2}, {"method": "ngram", "num_speculative_tokens": 0},
                {"method": "ngram", "num_speculative_tokens": 8}, {"method": "ngram"},
                {"method": "ngram", "num_speculative_tokens": 2, "model": "x"},
                {"method": "ngram", "num_speculative_tokens": 2, "prompt_lookup_max": 2, "prompt_lookup_min": 3}):
        with pytest.raises(ValueError):
            EngineConfig.create("tiny-llama", device="cpu", speculative_config=bad)
    p = add_engine_args(argparse.ArgumentParser())
    a = p.parse_args(["--model", "tiny-llama", "--device", "cpu", "--speculative-config", json.dumps(SPEC)])
    assert engine_config_from_args(a).speculative_config == SPEC
    assert engine_config_from_args(p.parse_args(["--device", "cpu"])).speculative_config is None


@pytest.mark.parametrize("model,kw,word", [
    ("tiny-deepseek", {}, "MLA"),
    ("tiny-gpt-oss", {}, "hybrid"),
    ("tiny-llama", {"tensor_parallel_size": 2}, "tensor parallelism"),
    ("tiny-llama", {"data_parallel_size": 2}, "data parallelism"),
    ("tiny-moe", {"enable_expert_parallel": True}, "wide-EP"),
    ("tiny-llama", {"enable_dbo": True}, "dual-batch"),
    ("tiny-llama", {"kv_transfer_config": {"kv_connector": "NixlConnector", "kv_role": "kv_both"}}, "KV connector"),
])
def test_startup_refusals(model, kw, word):
    cfg = EngineConfig.create(model, device="cpu", block_size=16, num_gpu_blocks=32, max_num_batched_tokens=64,
                              max_model_len=128, enforce_eager=True, speculative_config=SPEC, **kw)
    with pytest.raises(ValueError, match=word):
        LLMEngine(cfg)


# ---------------------------------------------------------------- HTTP
def test_http_streamed_completion_with_flag(base):
    from llmd_amd.serving.api_server import build_server

    def cfg(flag):
        argv = ["--model", "tiny-llama", "--device", "cpu", "--block-size", "16", "--num-gpu-blocks-override", "64",
                "--max-num-batched-tokens", "128", "--max-num-seqs", "4", "--max-model-len", "256",
                "--enforce-eager"]
        if flag:
            argv += ["--speculative-config", json.dumps(SPEC)]
        return engine_config_from_args(add_engine_args(argparse.ArgumentParser()).parse_args(argv))

    async def run(flag):
        srv = build_server(cfg(flag))
        runner = web.AppRunner(srv.app(), access_log=None)
        await runner.setup()
        site = web.TCPSite(runner, "127.0.0.1", 0)
        await site.start()
        port = site._server.sockets[0].getsockname()[1]
        try:
            async with aiohttp.ClientSession() as s:
                async with s.post(f"http://127.0.0.1:{port}/v1/completions",
                                  json={"prompt": REPEATING, "max_tokens": 32, "temperature": 0, "ignore_eos": True,
                                        "stream": True, "stream_options": {"include_usage": True}}) as r:
                    assert r.status == 200
                    text = await r.text()
            chunks = [json.loads(l[5:]) for l in text.splitlines() if l.startswith("data:") and "[DONE]" not in l]
            spec = srv.aeng.engine.spec
            return ("".join(ch["text"] for c in chunks for ch in c["choices"]),
                    chunks[-1]["usage"]["completion_tokens"], spec.num_accepted_tokens if spec else None)
        finally:
            await runner.cleanup()
            srv.aeng.shutdown()

    t0, n0, _ = asyncio.run(run(False))
    t1, n1, acc = asyncio.run(run(True))
    assert (t1, n1) == (t0, n0) and n0 == 32 and acc > 0
