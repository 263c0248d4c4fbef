"""Prompt scoring (`prompt_logprobs`, `echo`): the CPU reference op against the kernel's contract,
the OpenAI request mapping, the CPU engine under every scheduling case, and the HTTP surface.
The oracle and the engine helpers are shared with tests/test_prompt_logprobs_gpu.py."""
import asyncio

import aiohttp
import numpy as np
import pytest
import torch

from llmd_amd import ops
from llmd_amd.engine.config import EngineConfig
from llmd_amd.engine.engine import LLMEngine
from llmd_amd.engine.request import SamplingParams
from llmd_amd.ops import reference as ref
from llmd_amd.serving.api_server import build_server
from test_top_logprobs import LP_ATOL, NEG_INF, NMAX, _serve, _sse, check_against_oracle, tie_rows


# ---------------------------------------------------------------- oracle of the op
def score_oracle(x, targets):
    """x: CPU rows in the tested dtype. lp from a float64 log-softmax, rank = (x >= x[t]).sum() on
    the stored values; a target outside [0, V) gives -inf / 0, a -inf target -inf / V."""
    R, V = x.shape
    logp = torch.log_softmax(x.double(), -1)
    lp = torch.full((R,), NEG_INF, dtype=torch.float64)
    rank = torch.zeros(R, dtype=torch.int64)
    for r, t in enumerate(targets):
        if 0 <= t < V:
            rank[r] = int((x[r] >= x[r, t]).sum())
            if x[r, t] > NEG_INF:
                lp[r] = logp[r, t]
    return lp, rank


def check_score(x_cpu, targets, n_per_row, got):
    """got = (lp, rank, top_ids, top_lp) of ops.prompt_logprobs on x_cpu's values."""
    lp, rank, ids, tlp = got
    R = x_cpu.shape[0]
    assert lp.dtype == torch.float32 and rank.dtype == torch.int32
    assert tuple(lp.shape) == tuple(rank.shape) == (R,)
    want_lp, want_rank = score_oracle(x_cpu, targets)
    assert rank.cpu().long().tolist() == want_rank.tolist()
    got_lp = lp.cpu().double()
    fin = want_lp > NEG_INF
    assert (got_lp[~fin] == NEG_INF).all()
    err = (got_lp[fin] - want_lp[fin]).abs().max().item() if fin.any() else 0.0
    print(f"prompt_logprobs {tuple(x_cpu.shape)} {x_cpu.dtype}: max |lp - float64| = {err:.3e}")
    assert err <= LP_ATOL, err
    check_against_oracle(x_cpu, n_per_row, ids, tlp)


# ---------------------------------------------------------------- reference op
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_reference_contract(dtype):
    V = 5003
    x = (torch.randn(6, V, generator=torch.Generator().manual_seed(0)) * 3).to(dtype)
    x[3, np.linspace(3, V - 4, 30).astype(int).tolist()] = 20.0   # thirty equal entries above the rest
    x[4, 77] = NEG_INF
    targets = [0, V - 1, V - 2, 3, 77, -1]   # V - 2: inside the scalar tail (5003 = 625 * 8 + 3)
    n = [1, 5, 20, 0, 20, 5]
    got = ops.prompt_logprobs(x, torch.tensor(targets, dtype=torch.int32), torch.tensor(n, dtype=torch.int32))
    check_score(x, targets, n, got)      # CPU tensors dispatch to the reference
    lp, rank, ids, tlp = got
    assert rank[3] == 30 and abs(lp[3].item() - tlp_of(x[3], 3)) <= LP_ATOL  # the ties all count
    assert lp[4] == NEG_INF and rank[4] == V
    assert lp[5] == NEG_INF and rank[5] == 0 and (ids[5, :5] >= 0).all()    # alternatives still reported
    assert (ids[3] == -1).all() and (tlp[3] == NEG_INF).all()
    got = ref.prompt_logprobs(x[:1], torch.tensor([V], dtype=torch.int32), torch.tensor([20], dtype=torch.int32))
    check_score(x[:1], [V], [20], got)
    assert got[0][0] == NEG_INF and got[1][0] == 0
    with pytest.raises(ValueError):
        ops.prompt_logprobs(x, torch.zeros(5, dtype=torch.int32), torch.zeros(6, dtype=torch.int32))


def tlp_of(row, t):
    return torch.log_softmax(row.double(), -1)[t].item()


def test_reference_ties_count_in_the_rank():
    """tie_rows: thirty 9.0s over a background below 7. A target among them is tied with 29
    others and has rank 30, wherever it sits."""
    x, want = tie_rows(128259, torch.bfloat16)
    targets = [want[0][-1], want[1][0], want[2][7], want[3][19]]
    n = [20, 0, 5, 20]
    got = ref.prompt_logprobs(x, torch.tensor(targets, dtype=torch.int32), torch.tensor(n, dtype=torch.int32))
    check_score(x, targets, n, got)
    assert got[1].tolist() == [30] * 4


# ---------------------------------------------------------------- request mapping
def test_from_openai_mapping():
    f = SamplingParams.from_openai
    assert f({}).prompt_logprobs is None and not f({}).scored
    assert f({"prompt_logprobs": 0}).prompt_logprobs == 0 and f({"prompt_logprobs": 0}).scored
    assert f({"prompt_logprobs": 20}).prompt_logprobs == 20
    assert f({"messages": [], "prompt_logprobs": 2}).prompt_logprobs == 2
    for bad in (-1, 21, True, 1.5, "2"):
        with pytest.raises(ValueError):
            f({"prompt_logprobs": bad})
    with pytest.raises(ValueError):
        SamplingParams(prompt_logprobs=21)._validated()
    with pytest.raises(ValueError):
        f({"echo": "yes"})
    with pytest.raises(ValueError, match="chat"):
        f({"messages": [{"role": "user", "content": "x"}], "echo": True})
    with pytest.raises(ValueError, match="stream"):
        f({"prompt_logprobs": 1, "stream": True})
    # echo: scores only with logprobs, with as many alternatives; it may stream
    sp = f({"echo": True, "logprobs": 3})
    assert sp.prompt_logprobs == 3 and sp.top_logprobs == 3 and sp.logprobs == 3
    assert f({"echo": True, "logprobs": 1, "stream": True}).prompt_logprobs == 1
    assert f({"echo": True}).prompt_logprobs is None
    assert f({"echo": False, "logprobs": 3}).prompt_logprobs is None
    assert f({"echo": True, "logprobs": 2, "prompt_logprobs": 5}).prompt_logprobs == 5
    # max_tokens 0: with echo the engine request generates one token (the server drops it);
    # without echo the mapping is what it was
    assert f({"echo": True, "max_tokens": 0}).max_tokens == 1
    assert f({"echo": True, "max_tokens": 0, "logprobs": 1}).max_tokens == 1
    assert f({"max_tokens": 0}).max_tokens == 0
    assert f({"echo": True, "max_tokens": 3}).max_tokens == 3


# ---------------------------------------------------------------- engine
P50 = np.random.default_rng(1).integers(3, 500, size=50).tolist()
P49 = np.random.default_rng(2).integers(3, 500, size=49).tolist()   # chunks of 16: an edge at P - 1 = 48
P67 = np.random.default_rng(3).integers(3, 500, size=67).tolist()
ENG_KW = dict(block_size=16, num_gpu_blocks=64, max_num_batched_tokens=256, max_num_seqs=8, max_model_len=256,
              enforce_eager=True, dtype="float32")


def make_engine(device="cpu", **kw):
    return LLMEngine(EngineConfig.create("tiny-llama", device=device, **dict(ENG_KW, **kw)))


def record_chunks(eng):
    """(start, tokens) of every request's chunk, per step, as the runner plans them."""
    steps, plan = [], eng.runner.plan

    def wrapped(so, bt):
        steps.append({s.req.request_id: (s.start, s.num_new_tokens) for s in so.all()})
        return plan(so, bt)
    eng.runner.plan = wrapped
    return steps


def run(eng):
    outs = []
    while eng.has_unfinished():
        outs.extend(eng.step())
    return outs


def scoring(n, max_tokens=2, **kw):
    return SamplingParams(max_tokens=max_tokens, temperature=0.0, ignore_eos=True, prompt_logprobs=n, **kw)


def prompt_logits(eng, prompt):
    """The engine oracle: one unchunked forward of eng's model over the whole prompt (fresh blocks,
    no cache hit), every row through compute_logits. [P, V] on the CPU, in the model's dtype."""
    from llmd_amd.engine.request import Request
    from llmd_amd.engine.scheduler import ScheduledReq, SchedulerOutput

    r = Request("oracle", list(prompt), SamplingParams(max_tokens=1))
    assert eng.bm.acquire(r.seq_id, np.asarray(prompt, dtype=np.int32), 0, 0) == 0
    assert eng.bm.grow(r.seq_id, len(prompt))
    so = SchedulerOutput(prefills=[ScheduledReq(r, len(prompt), 0)])
    pl, _ = eng.runner.plan(so, eng.block_tables(so))
    with torch.no_grad():
        ids, meta = eng.runner._eager_meta(pl)
        logits = eng.runner.model.compute_logits(eng.runner.model(ids, meta))
    eng.bm.free(r.seq_id)
    return logits.cpu()


def check_request(r, logits, n):
    """Request.prompt_logprobs against a float64 log-softmax of the oracle's rows: row i - 1 scores
    prompt token i. LP_ATOL, exact ranks and ids."""
    toks = r.prompt_token_ids
    P = len(toks)
    got = r.prompt_logprobs
    assert len(got) == P == r.num_prompt_tokens and got[0] is None
    assert all(e is not None and len(e) == 3 for e in got[1:])
    lp = torch.tensor([e[0] for e in got[1:]])
    rank = torch.tensor([e[1] for e in got[1:]], dtype=torch.int32)
    ids = torch.full((P - 1, NMAX), -1, dtype=torch.int32)
    tlp = torch.full((P - 1, NMAX), NEG_INF)
    for i, e in enumerate(got[1:]):
        assert len(e[2]) == n
        ids[i, :n] = torch.tensor([t for t, _ in e[2]], dtype=torch.int32)
        tlp[i, :n] = torch.tensor([l for _, l in e[2]])
    check_score(logits[:P - 1], toks[1:], [n] * (P - 1), (lp, rank, ids, tlp))


@pytest.fixture(scope="module")
def oracle50():
    eng = make_engine()
    return {tuple(p): prompt_logits(eng, p) for p in (P50, P49, P67)}


def test_engine_one_chunk(oracle50):
    eng = make_engine()
    r = eng.add_request("s", P50, scoring(5))
    outs = run(eng)
    check_request(r, oracle50[tuple(P50)], 5)
    # delivered once, with the output that carries the first generated token
    mine = [o for o in outs if o.request_id == "s"]
    assert len(mine) == 2 and mine[0].prompt_logprobs is r.prompt_logprobs and mine[1].prompt_logprobs is None
    assert mine[0].num_output_tokens == 1
    assert b'llmd:prompt_tokens_scored_total{model_name="tiny-llama"} 49.0' in eng.metrics.render()
    # an unscored request: nothing anywhere
    q = eng.add_request("q", P50, SamplingParams(max_tokens=1, temperature=0.0))
    assert all(o.prompt_logprobs is None for o in run(eng)) and q.prompt_logprobs is None


def test_engine_chunked_warm_cache_and_neighbours(oracle50):
    """(b) chunks [0,16) [16,32) [32,48) [48,49): an edge at P - 1; (c) the same prompt with a warm
    cache takes no hit and gives the same values; (d) an unscored request afterwards still hits."""
    eng = make_engine(max_num_batched_tokens=16)
    steps = record_chunks(eng)
    cold = eng.add_request("cold", P49, scoring(3))
    run(eng)
    assert [c["cold"] for c in steps[:4]] == [(0, 16), (16, 16), (32, 16), (48, 1)]
    check_request(cold, oracle50[tuple(P49)], 3)
    assert eng.bm.lookup(np.asarray(P49, dtype=np.int32), 0) == 48   # its blocks were committed
    warm = eng.add_request("warm", P49, scoring(3))
    run(eng)
    assert warm.num_cached_tokens == 0
    assert warm.prompt_logprobs == cold.prompt_logprobs
    assert warm.output_token_ids == cold.output_token_ids
    plain = eng.add_request("plain", P49, SamplingParams(max_tokens=2, temperature=0.0, ignore_eos=True))
    run(eng)
    assert plain.num_cached_tokens == 48 and plain.prompt_logprobs is None
    assert plain.output_token_ids == cold.output_token_ids


def test_engine_preempted_mid_prompt(oracle50):
    """(e) preempted after two chunks: the recompute overwrites by position - one entry each."""
    from llmd_amd.engine.scheduler import SchedulerOutput

    eng = make_engine(max_num_batched_tokens=16)
    r = eng.add_request("s", P67, scoring(2))
    eng.step()
    eng.step()
    eng.drain()
    assert r.num_computed_tokens == 32 and r.prompt_logprobs[32] is not None and r.prompt_logprobs[33] is None
    eng.sched._preempt(r, SchedulerOutput())
    assert r.num_computed_tokens == 0
    run(eng)
    assert r.num_preemptions == 1 and len(r.output_token_ids) == 2
    check_request(r, oracle50[tuple(P67)], 2)
    assert eng.runner.num_scored == 32 + 66


def test_engine_one_token_chunk_mid_prompt(oracle50):
    """A neighbour's chunk leaves one token of the step's budget: the scored prompt's first chunk
    is a single token, which the scheduler lists among the decode rows. It is scored all the same."""
    eng = make_engine(max_num_batched_tokens=16)
    steps = record_chunks(eng)
    eng.add_request("first", P50[:15], SamplingParams(max_tokens=1, temperature=0.0))
    r = eng.add_request("s", P49, scoring(2))
    run(eng)
    assert steps[0]["s"] == (0, 1)
    check_request(r, oracle50[tuple(P49)], 2)


@pytest.mark.parametrize("async_on", [True, False])
def test_engine_mixed_batch(oracle50, async_on):
    """(f) scored, plain, penalised and guided requests in one batch: the scores are the oracle's
    (raw log-softmax: the scored request's own temperature, top-k and bias change nothing), and
    the others' tokens are those of a run without the scored request."""
    from llmd_amd.guided import TokenTable, compile_regex
    from llmd_amd.serving.tokenizer import ByteTokenizer

    greedy = dict(max_tokens=6, temperature=0.0, ignore_eos=True)
    jobs = {
        "plain": (P50[:20], SamplingParams(**greedy)),
        "penalised": (P67[:23], SamplingParams(presence_penalty=0.5, **greedy)),
        "guided": (P49[:17], SamplingParams(max_tokens=6, temperature=0.0, guided=compile_regex(r"[a-c]{30}"))),
    }
    res = {}
    for with_scored in (False, True):
        eng = make_engine(max_num_batched_tokens=32, async_scheduling=async_on)
        assert eng.async_sched == async_on
        eng.set_token_table(TokenTable(*ByteTokenizer(512).token_bytes(512)))
        reqs = {n: eng.add_request(n, p, sp) for n, (p, sp) in jobs.items()}
        if with_scored:
            s = eng.add_request("s", P67, scoring(4, max_tokens=6, logit_bias={5: 50.0}))
            t = eng.add_request("t", P50, SamplingParams(max_tokens=6, temperature=0.7, top_k=3, seed=1,
                                                         ignore_eos=True, prompt_logprobs=0))
        run(eng)
        res[with_scored] = {n: list(r.output_token_ids) for n, r in reqs.items()}
        assert all(len(v) == 6 and -1 not in v for v in res[with_scored].values())
    check_request(s, oracle50[tuple(P67)], 4)
    check_request(t, oracle50[tuple(P50)], 0)
    assert res[True] == res[False]


def test_engine_with_ngram_speculation(oracle50):
    """(g) drafts start after the prompt: scoring needs no special case."""
    spec = {"method": "ngram", "num_speculative_tokens": 4, "prompt_lookup_max": 4, "prompt_lookup_min": 2}
    eng = make_engine(max_num_batched_tokens=32, speculative_config=spec)
    assert eng.spec is not None
    r = eng.add_request("s", P67, scoring(1, max_tokens=12))
    rep = eng.add_request("rep", [7, 8, 9] * 5, SamplingParams(max_tokens=24, temperature=0.0, ignore_eos=True))
    run(eng)
    check_request(r, oracle50[tuple(P67)], 1)
    assert len(r.output_token_ids) == 12 and len(rep.output_token_ids) == 24 and eng.spec.num_drafts > 0


def test_engine_refusals():
    eng = make_engine()
    sp = scoring(1)
    with pytest.raises(ValueError, match="kv_transfer_params"):
        eng.add_request("a", P50, sp, kv_transfer_params={"do_remote_decode": True})
    with pytest.raises(ValueError, match="multimodal"):
        eng.add_request("b", P50, sp, mm_inputs=[object()])
    with pytest.raises(ValueError, match="embed"):
        eng.add_request("c", P50, scoring(1, embed=True))
    for attr, val, why in (("tensor_parallel_size", 2, "TP > 1"), ("data_parallel_size", 2, "wide-EP"),
                           ("enable_dbo", True, "dual-batch")):
        old = getattr(eng.cfg.parallel, attr)
        setattr(eng.cfg.parallel, attr, val)
        with pytest.raises(ValueError, match=why):
            eng.add_request("d", P50, sp)
        setattr(eng.cfg.parallel, attr, old)
    eng.connector = object()
    with pytest.raises(ValueError, match="KV connector"):
        eng.add_request("e", P50, sp)
    eng.connector = None
    assert not eng.sched.requests
    eng.add_request("ok", P50, sp)                       # and an unscored request is never refused for these
    eng.cfg.parallel.enable_dbo = True
    eng.add_request("plain", P50, SamplingParams(max_tokens=1))


# ---------------------------------------------------------------- HTTP
CTX = np.random.default_rng(5).integers(35, 126, size=24).tolist()   # ASCII bytes: one string per id
MSGS = [{"role": "user", "content": "hi"}]


@pytest.fixture(scope="module")
def http():
    """One server, every request of the HTTP tests, answers by name. The scored prompt is CTX plus
    the model's own greedy continuation of it, so that some of its tokens have rank 1."""
    async def main():
        srv = build_server(EngineConfig.create("tiny-llama", device="cpu", **dict(ENG_KW, num_gpu_blocks=128)))
        eng = srv.aeng.engine
        r1, port = await _serve(srv.app())
        comp = f"http://127.0.0.1:{port}/v1/completions"
        chat = f"http://127.0.0.1:{port}/v1/chat/completions"
        out = {"tok": srv.tok}
        try:
            async with aiohttp.ClientSession() as s:
                async def post(name, url, body, sse=False):
                    async with s.post(url, json=body) as r:
                        out[name + "_status"] = r.status
                        out[name] = _sse(await r.text()) if sse else await r.json()
                await post("gen", comp, {"prompt": CTX, "max_tokens": 16, "temperature": 0, "ignore_eos": True,
                                         "return_token_ids": True})
                full = out["full"] = CTX + out["gen"]["choices"][0]["token_ids"]
                await post("lmeval", comp, {"prompt": full, "max_tokens": 1, "temperature": 0, "logprobs": 1,
                                            "echo": True})
                await post("plp1", comp, {"prompt": full, "max_tokens": 1, "temperature": 0, "prompt_logprobs": 1,
                                          "return_token_ids": True})
                await post("chat2", chat, {"messages": MSGS, "prompt_logprobs": 2, "max_tokens": 3, "temperature": 0})
                n0 = eng.runner.num_scored
                await post("n2", comp, {"prompt": full, "n": 2, "prompt_logprobs": 1, "max_tokens": 2,
                                        "temperature": 0.8, "seed": 3})
                out["n2_scored"] = eng.runner.num_scored - n0
                await post("echo_stream", comp, {"prompt": full, "echo": True, "logprobs": 1, "stream": True,
                                                 "max_tokens": 3, "temperature": 0, "ignore_eos": True,
                                                 "stream_options": {"include_usage": True}}, sse=True)
                await post("echo0", comp, {"prompt": full, "echo": True, "logprobs": 1, "max_tokens": 0})
                n0 = eng.runner.num_scored
                await post("echo_plain", comp, {"prompt": "hello", "echo": True, "max_tokens": 3, "temperature": 0,
                                                "ignore_eos": True, "return_token_ids": True})
                await post("echo_plain_stream", comp, {"prompt": "hello", "echo": True, "max_tokens": 3,
                                                       "temperature": 0, "ignore_eos": True, "stream": True}, sse=True)
                await post("echo0_plain", comp, {"prompt": "hello", "echo": True, "max_tokens": 0})
                out["plain_scored"] = eng.runner.num_scored - n0
                for name, url, body in (
                        ("bad_range", comp, {"prompt": full, "prompt_logprobs": 21}),
                        ("bad_neg", comp, {"prompt": full, "prompt_logprobs": -1}),
                        ("bad_type", comp, {"prompt": full, "prompt_logprobs": "2"}),
                        ("bad_bool", chat, {"messages": MSGS, "prompt_logprobs": True}),
                        ("bad_stream", comp, {"prompt": full, "prompt_logprobs": 1, "stream": True}),
                        ("bad_chat_stream", chat, {"messages": MSGS, "prompt_logprobs": 1, "stream": True}),
                        ("bad_echo", comp, {"prompt": full, "echo": "yes"}),
                        ("bad_chat_echo", chat, {"messages": MSGS, "echo": True}),
                        ("bad_ktp", comp, {"prompt": full, "prompt_logprobs": 1,
                                           "kv_transfer_params": {"do_remote_decode": True}})):
                    await post(name, url, dict(body, max_tokens=1))
                # engines that cannot score say why
                eng.cfg.parallel.tensor_parallel_size = 2
                await post("tp", comp, {"prompt": full, "prompt_logprobs": 1})
                await post("tp_echo", comp, {"prompt": full, "echo": True, "logprobs": 1})
                await post("tp_unscored", comp, {"prompt": full, "echo": True, "max_tokens": 1})
                eng.cfg.parallel.tensor_parallel_size = 1
                eng.cfg.kv_transfer_config = {"kv_connector": "NixlConnector"}
                await post("pd", comp, {"prompt": full, "prompt_logprobs": 1})
                eng.cfg.kv_transfer_config = None

                async def fake_mm(body, headers):
                    return srv._chat_ids(body), [object()]
                srv.mm, srv._has_images, srv._chat_mm = object(), lambda body: True, fake_mm
                await post("mm", chat, {"messages": MSGS, "prompt_logprobs": 1})
                srv.mm = None
                del srv._has_images, srv._chat_mm
            out["logits"] = await srv.aeng.call(lambda e: prompt_logits(e, full))
            return out
        finally:
            await r1.cleanup()
            srv.aeng.shutdown()

    return asyncio.run(main())


def _want_lps(http):
    full = http["full"]
    logp = torch.log_softmax(http["logits"].double(), -1)
    return [logp[i - 1, t].item() for i, t in enumerate(full) if i > 0]


def test_http_lm_eval_loglikelihood(http):
    """lm-eval's local-completions request: a token-id prompt, max_tokens 1, logprobs 1, echo. It
    reads token_logprobs[ctxlen:-1] and, per position, whether the likeliest key of top_logprobs
    is the token."""
    full, tok, ctxlen = http["full"], http["tok"], len(CTX)
    P = len(full)
    assert http["lmeval_status"] == 200 and P == 40
    ch = http["lmeval"]["choices"][0]
    lp = ch["logprobs"]
    assert set(lp) == {"tokens", "token_logprobs", "top_logprobs", "text_offset"}
    assert all(len(lp[k]) == P + 1 for k in lp)
    assert lp["token_logprobs"][0] is None and lp["top_logprobs"][0] is None
    strs = [tok.decode([t]) for t in full]
    assert lp["tokens"][:P] == strs and ch["text"] == tok.decode(full) + lp["tokens"][P]
    assert lp["text_offset"] == [sum(len(s) for s in lp["tokens"][:i]) for i in range(P + 1)]
    assert http["lmeval"]["usage"] == {"prompt_tokens": P, "completion_tokens": 1, "total_tokens": P + 1}
    want = _want_lps(http)
    got = lp["token_logprobs"][1:P]
    err = max(abs(a - b) for a, b in zip(got, want))
    print(f"echo token_logprobs against the float64 oracle: max error {err:.3e}")
    assert err <= LP_ATOL
    assert lp["token_logprobs"][ctxlen:-1] == got[ctxlen - 1:]     # the slice lm-eval sums
    # is_greedy lm-eval's way against the rank of the same position (vLLM's prompt_logprobs). Two
    # kinds of position cannot be compared: where the row's maximum is not unique (the rank counts
    # the ties, the argmax takes the lower index), and where the likeliest id and the prompt's
    # decode to one string (the byte tokenizer gives "" to every id past its 256 bytes), which the
    # string-keyed OpenAI object cannot tell apart
    x = http["logits"]
    checked = 0
    for i in range(ctxlen, P):
        d = http["plp1"]["choices"][0]["prompt_logprobs"][i]
        rank = d[str(full[i])]["rank"]
        assert rank == int((x[i - 1] >= x[i - 1, full[i]]).sum())
        top = lp["top_logprobs"][i]
        assert 1 <= len(top) <= 2 and top[strs[i]] == lp["token_logprobs"][i]
        is_greedy = max(top.keys(), key=lambda k: top[k]) == lp["tokens"][i]
        if int((x[i - 1] == x[i - 1].max()).sum()) == 1 and len({e["decoded_token"] for e in d.values()}) == len(d):
            assert is_greedy == (rank == 1), i
            checked += rank == 1
    assert checked >= 6   # the continuation is the model's own greedy one


def test_http_prompt_logprobs_shape(http):
    full, tok, x = http["full"], http["tok"], http["logits"]
    ch = http["plp1"]["choices"][0]
    plp = ch["prompt_logprobs"]
    assert len(plp) == len(full) and plp[0] is None and "logprobs" not in ch
    want = _want_lps(http)
    for i, (t, d, w) in enumerate(zip(full[1:], plp[1:], want)):
        keys = list(d)
        assert keys[0] == str(t) and 1 <= len(keys) <= 2      # the prompt token first, never repeated
        for k, e in d.items():
            assert set(e) == {"logprob", "rank", "decoded_token"} and e["decoded_token"] == tok.decode([int(k)])
        own = d[str(t)]
        assert abs(own["logprob"] - w) <= LP_ATOL and own["rank"] == int((x[i] >= x[i, t]).sum())
        if len(keys) == 2:  # the likeliest token is another one
            assert d[keys[1]]["rank"] == 1 and own["rank"] > 1 and d[keys[1]]["logprob"] >= own["logprob"]
            assert int(keys[1]) == int(x[i].argmax())
        else:               # it is the prompt's own (rank 1, or more where others tie with it)
            assert x[i, t] == x[i].max()
    # chat: the rendered prompt's tokens with two alternatives each
    plp = http["chat2"]["choices"][0]["prompt_logprobs"]
    assert http["chat2_status"] == 200 and len(plp) == http["chat2"]["usage"]["prompt_tokens"] > 2
    assert plp[0] is None
    for d in plp[1:]:
        ents = list(d.values())
        assert 2 <= len(ents) <= 3 and all(np.isfinite(e["logprob"]) and e["rank"] >= 1 for e in ents)
        others = [e["rank"] for e in ents[1:]]           # rank = place among the two alternatives
        # three entries: the prompt's token is neither alternative; two: it is one of them
        assert others == [1, 2] if len(ents) == 3 else others in ([1], [2])
        assert ents[1]["logprob"] >= ents[-1]["logprob"]


def test_http_n_scores_once(http):
    """n = 2: sample 0 scores the prompt, the result serves both choices."""
    a, b = http["n2"]["choices"]
    assert a["prompt_logprobs"] == b["prompt_logprobs"] == http["plp1"]["choices"][0]["prompt_logprobs"]
    assert http["n2_scored"] == len(http["full"]) - 1


def test_http_echo_stream_and_max_tokens_0(http):
    full, tok = http["full"], http["tok"]
    P = len(full)
    chunks = http["echo_stream"]
    first = next(c for c in chunks if c["choices"])
    assert first["choices"][0]["text"].startswith(tok.decode(full))
    lps = [ch["logprobs"] for c in chunks for ch in c["choices"] if ch.get("logprobs")]
    assert lps[0]["token_logprobs"][0] is None and lps[0]["top_logprobs"][0] is None
    assert lps[0]["tokens"][:P] == [tok.decode([t]) for t in full]
    toks = [t for l in lps for t in l["tokens"]]
    assert len(toks) == P + 3 and chunks[-1]["usage"]["completion_tokens"] == 3
    assert [o for l in lps for o in l["text_offset"]] == [sum(len(s) for s in toks[:i]) for i in range(P + 3)]
    assert "".join(ch["text"] for c in chunks for ch in c["choices"]) == "".join(toks)
    ref_lp = http["lmeval"]["choices"][0]["logprobs"]["token_logprobs"][1:P]
    assert [l for l in lps[0]["token_logprobs"][1:P]] == ref_lp
    # max_tokens 0: the prompt alone, the engine's one token dropped everywhere
    e0 = http["echo0"]
    ch = e0["choices"][0]
    assert http["echo0_status"] == 200 and ch["text"] == tok.decode(full)
    assert all(len(v) == P for v in ch["logprobs"].values()) and ch["logprobs"]["token_logprobs"][1:] == ref_lp
    assert e0["usage"] == {"prompt_tokens": P, "completion_tokens": 0, "total_tokens": P}
    # echo without logprobs: the text only, and nothing was scored
    ch = http["echo_plain"]["choices"][0]
    assert len(ch["token_ids"]) == 3 and ch["text"] == "hello" + tok.decode(ch["token_ids"]) and "logprobs" not in ch
    assert "".join(c["choices"][0]["text"] for c in http["echo_plain_stream"] if c["choices"]) == ch["text"]
    assert http["echo0_plain"]["choices"][0]["text"] == "hello"
    assert http["echo0_plain"]["usage"]["completion_tokens"] == 0
    assert http["plain_scored"] == 0


def test_http_400s_and_refusing_engines(http):
    for name in ("bad_range", "bad_neg", "bad_type", "bad_bool", "bad_stream", "bad_chat_stream", "bad_echo",
                 "bad_chat_echo", "bad_ktp"):
        assert http[name + "_status"] == 400, name
    assert "stream" in http["bad_stream"]["error"]["message"]
    assert "kv_transfer_params" in http["bad_ktp"]["error"]["message"]
    for name, why in (("tp", "TP > 1"), ("tp_echo", "TP > 1"), ("pd", "KV connector"), ("mm", "multimodal")):
        assert http[name + "_status"] == 400 and why in http[name]["error"]["message"], name
    assert http["tp_unscored_status"] == 200   # echo without logprobs computes nothing: not refused
