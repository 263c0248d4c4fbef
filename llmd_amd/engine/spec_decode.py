"""Speculative decoding: draft proposals for running requests (SURVEY: vLLM ``--speculative-config``).

A running request with one token left to compute may carry ``k`` draft tokens into its step
(scheduler.py); the step computes the last real token and the drafts as ``1 + k`` rows whose
attention is one ``ops.paged_verify`` pass, every row is sampled with the ordinary sampler, and
the longest prefix of drafts that equals the sampled tokens is accepted: the request then emits
``n_acc + 1`` tokens in one step. There is no rejection sampler - an accepted draft IS the token
the sampler produced at its position, so greedy outputs are exactly those of plain decoding, and
so are seeded GPU samples (the GPU sampler's Gumbel keys depend only on (seed, vocabulary index),
and row ``j`` gets the seed of output length ``len + j``). The CPU reference sampler draws every
row of a step from one generator and therefore keeps only the distribution.

The proposer is n-gram prompt lookup: no second model. ``NgramIndex`` (native in
``csrc/runtime/ngram.cpp``, the Python class below for builds without ``_rt``) maps every n-gram,
``prompt_lookup_min <= n <= prompt_lookup_max``, of a request's prompt + output to the position
after its most recent occurrence; a proposal is what followed the longest suffix n-gram.
``SpecDecode.proposer`` is pluggable: any ``callable(request, k) -> list[int]``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional

MAX_SPECULATIVE_TOKENS = 7  # ops.paged_verify attends at most 8 rows per sequence


@dataclass
class SpeculativeConfig:
    method: str = "ngram"
    num_speculative_tokens: int = 4
    prompt_lookup_max: int = 4
    prompt_lookup_min: int = 2

    @classmethod
    def from_dict(cls, d: Optional[dict]) -> Optional["SpeculativeConfig"]:
        """vLLM's ``--speculative-config`` JSON. ValueError for anything this engine cannot run."""
        if not d:
            return None
        if not isinstance(d, dict):
            raise ValueError(f"speculative_config must be a JSON object, got {type(d).__name__}")
        known = {"method", "num_speculative_tokens", "prompt_lookup_max", "prompt_lookup_min"}
        unknown = sorted(set(d) - known)
        if unknown:
            raise ValueError(f"speculative_config: unsupported keys {unknown} (supported: {sorted(known)})")
        method = d.get("method", "ngram")
        if method != "ngram":
            raise ValueError(f"speculative_config: method {method!r} is not supported; the only draft "
                             "method is 'ngram' (prompt lookup, no draft model)")
        if "num_speculative_tokens" not in d:
            raise ValueError("speculative_config: num_speculative_tokens is required")
        k = d["num_speculative_tokens"]
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_SPECULATIVE_TOKENS:
            raise ValueError(f"speculative_config: num_speculative_tokens must be an integer in "
                             f"[1, {MAX_SPECULATIVE_TOKENS}], got {k!r}")
        hi, lo = d.get("prompt_lookup_max"), d.get("prompt_lookup_min")
        if hi is None and lo is None:
            hi, lo = 4, 2
        elif hi is None:  # vLLM: one bound given sets both
            hi = lo
        elif lo is None:
            lo = hi
        for name, v in (("prompt_lookup_max", hi), ("prompt_lookup_min", lo)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"speculative_config: {name} must be a positive integer, got {v!r}")
        if lo > hi:
            raise ValueError(f"speculative_config: prompt_lookup_min {lo} above prompt_lookup_max {hi}")
        return cls(method, k, hi, lo)


class PyNgramIndex:
    """The interface of ``_rt.NgramIndex`` in Python (exact tuple keys instead of hashes)."""

    def __init__(self, min_n: int, max_n: int):
        if min_n < 1 or max_n < min_n:
            raise ValueError("NgramIndex: need 1 <= min_n <= max_n")
        self.min_n, self.max_n = min_n, max_n
        self.toks: list[int] = []
        self.map: dict[tuple, int] = {}

    def append(self, tokens) -> None:
        toks, mp = self.toks, self.map
        for t in tokens:
            i = len(toks)  # the n-grams ending at token i - 1 gain a successor: register them
            for n in range(self.min_n, min(self.max_n, i) + 1):
                mp[tuple(toks[i - n:i])] = i
            toks.append(int(t))

    def propose(self, k: int) -> list[int]:
        toks = self.toks
        ln = len(toks)
        if k <= 0:
            return []
        for n in range(min(self.max_n, ln), self.min_n - 1, -1):
            pos = self.map.get(tuple(toks[ln - n:]))
            if pos is not None:
                return toks[pos:min(ln, pos + k)]
        return []

    def __len__(self) -> int:
        return len(self.toks)


def make_ngram_index(min_n: int, max_n: int, native: Optional[bool] = None):
    """The native index, or the Python one when ``_rt`` is not built (``native=False`` forces it)."""
    if native is not False:
        try:
            from llmd_amd import _rt_loader

            return _rt_loader.rt().NgramIndex(min_n, max_n)
        except Exception:  # noqa: BLE001 - no compiler / no _rt: the Python class has the same interface
            if native:
                raise
    return PyNgramIndex(min_n, max_n)


class NgramProposer:
    """callable(request, k): one index per request, created at its first proposal, extended by
    the tokens it gained since, dropped when it finishes or is preempted (recompute rebuilds it)."""

    def __init__(self, sc: SpeculativeConfig):
        self.sc = sc
        self.index: dict[int, object] = {}

    def __call__(self, r, k: int) -> list[int]:
        ix = self.index.get(r.seq_id)
        if ix is None:
            ix = self.index[r.seq_id] = make_ngram_index(self.sc.prompt_lookup_min, self.sc.prompt_lookup_max)
            ix.append(r.prompt_token_ids)
        n = len(ix) - len(r.prompt_token_ids)
        if n < len(r.output_token_ids):
            ix.append(r.output_token_ids[n:])
        return list(ix.propose(k))

    def drop(self, r) -> None:
        self.index.pop(r.seq_id, None)


class SpecDecode:
    """Per-engine speculation state: the config, the proposer and the step counters the metrics read."""

    def __init__(self, sc: SpeculativeConfig):
        self.sc = sc
        self.k = sc.num_speculative_tokens
        self.proposer: Callable = NgramProposer(sc)
        self.num_drafts = 0
        self.num_draft_tokens = 0
        self.num_accepted_tokens = 0
        self.accepted_per_pos = [0] * self.k

    def propose(self, r, k: int) -> list[int]:
        d = self.proposer(r, k)
        return [int(t) for t in d[:k]] if d else []

    def drop(self, r) -> None:
        drop = getattr(self.proposer, "drop", None)
        if drop is not None:
            drop(r)

    def record(self, n_draft: int, n_acc: int) -> None:
        self.num_drafts += 1
        self.num_draft_tokens += n_draft
        self.num_accepted_tokens += n_acc
        for j in range(n_acc):
            self.accepted_per_pos[j] += 1
