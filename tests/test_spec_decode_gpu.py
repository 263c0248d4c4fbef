"""Speculative decoding end to end on the GPU (tiny-llama bf16): verify steps through
ops.paged_verify reproduce the spec-off engine's greedy outputs.

A verify step computes a position as one of 1 + k rows of an eager step, the spec-off engine as a
single row of a replayed decode graph: other GEMM shapes and another attention kernel, so on a
random-init model a greedy argmax may flip between two near-equal bf16 logits (tests/greedy_check.py).
The cap below was set against the two paths the engine already had: spec-off with graphs versus
spec-off with enforce_eager=True on these prompts diverge on 0 of the 8 sequences."""
import numpy as np
import pytest

from llmd_amd.engine.config import EngineConfig
from llmd_amd.engine.engine import LLMEngine
from llmd_amd.engine.request import SamplingParams
from llmd_amd.engine.spec_decode import NgramProposer

from greedy_check import assert_greedy_match

pytestmark = pytest.mark.gpu

NTOK = 48
K = 4
SPEC = {"method": "ngram", "num_speculative_tokens": K, "prompt_lookup_max": 4, "prompt_lookup_min": 2}
MAX_DIVERGING = 2  # of 8 sequences, near-ties included


def prompts():
    rng = np.random.default_rng(7)
    out = [rng.integers(3, 500, n).tolist() for n in (5, 17, 33, 64, 100, 150)]
    return out + [[7, 8, 9] * 5, [3, 4, 5, 6] * 20]


def engine(spec=None, **kw):
    return LLMEngine(EngineConfig.create("tiny-llama", device="cuda", block_size=16, num_gpu_blocks=256,
                                         max_num_batched_tokens=512, max_num_seqs=16, max_model_len=512,
                                         speculative_config=spec, **kw))


@pytest.fixture(scope="module")
def ref_run():
    ref = engine()
    sp = SamplingParams(max_tokens=NTOK, temperature=0.0, ignore_eos=True)
    want = [r.output_token_ids for r in ref.generate(prompts(), sp)]
    return ref, want, sp


def test_oracle_and_ngram_drafts_match_spec_off(ref_run):
    ref, want, sp = ref_run
    by = {tuple(p): w for p, w in zip(prompts(), want)}

    def oracle(r, k):
        n = len(r.output_token_ids)
        return by[tuple(r.prompt_token_ids)][n:n + k]

    eng = engine(SPEC)
    assert not eng.async_sched
    eng.spec.proposer = oracle
    got = [r.output_token_ids for r in eng.generate(prompts(), sp)]
    div = assert_greedy_match(ref, prompts(), got, want)
    print("oracle drafts: diverging sequences", len(div), div, "accepted", eng.spec.num_accepted_tokens,
          "of", eng.spec.num_draft_tokens, "steps", eng.step_count)
    assert len(div) <= MAX_DIVERGING
    assert eng.spec.num_accepted_tokens > 0 and eng.step_count < NTOK

    # the real proposer, and drafts that are wrong after one token, on the same engine
    for prop in (NgramProposer(eng.spec.sc), lambda r, k: [t if j < 1 else (t + 1) % 512
                                                           for j, t in enumerate(oracle(r, k))]):
        eng.spec.proposer = prop
        n0 = eng.spec.num_drafts
        got = [r.output_token_ids for r in eng.generate(prompts(), sp)]
        div = assert_greedy_match(ref, prompts(), got, want)
        print("diverging sequences", len(div), div, "drafts", eng.spec.num_drafts - n0)
        assert len(div) <= MAX_DIVERGING and eng.spec.num_drafts > n0
