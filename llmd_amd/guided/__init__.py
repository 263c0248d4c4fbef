"""Structured outputs: guided choice, regex and JSON-schema decoding.

``compiler``   regex / choice / JSON schema -> byte-level DFA (``Grammar``), LRU cached
``TokenTable`` the bytes of every token id, what the mask kernel walks through the DFA
``from_request`` the constraint of an OpenAI / vLLM request body, compiled

The engine masks the logits of a constrained request with ``ops.guided_mask`` (csrc/ops/guided.hip)
and advances the request's DFA state by every token it accepts.
"""
from __future__ import annotations

import json
from typing import Optional

import numpy as np

from .compiler import (HARD_MAX_STATES, MAX_STATES, Grammar, compile_choice, compile_grammar,  # noqa: F401
                       compile_json_schema, compile_regex)


class TokenTable:
    """Flat uint8 bytes + int32 offsets ``[V + 1]``: token ``t`` is ``data[off[t]:off[t + 1]]``.
    Length-0 tokens (special tokens, ids without a byte meaning) are never allowed under a
    constraint."""

    def __init__(self, data: np.ndarray, offsets: np.ndarray):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        if offsets.ndim != 1 or offsets.size < 1 or offsets[0] != 0 or offsets[-1] != data.size \
                or (np.diff(offsets) < 0).any():
            raise ValueError("token table offsets must rise from 0 to the number of bytes")
        self.data, self.offsets = data, offsets
        self.vocab_size = offsets.size - 1
        self._dev: dict = {}

    def token(self, t: int) -> bytes:
        if not 0 <= t < self.vocab_size:
            return b""
        return self.data[self.offsets[t]:self.offsets[t + 1]].tobytes()

    def missing_bytes(self) -> list[int]:
        """Byte values that no single-byte token spells."""
        lens = np.diff(self.offsets)
        have = np.zeros(256, dtype=bool)
        have[self.data[self.offsets[:-1][lens == 1]]] = True
        return np.flatnonzero(~have).tolist()

    def check_guidable(self) -> "TokenTable":
        """With a single-byte token for each of the 256 byte values, every live DFA state has
        an allowed token (or is accepting), so no row can be fully masked."""
        miss = self.missing_bytes()
        if miss:
            raise ValueError("this tokenizer cannot serve guided requests: it has no single-byte token for "
                             f"{len(miss)} byte value(s), e.g. 0x{miss[0]:02x}")
        return self

    def on_device(self, device):
        """(bytes, offsets) tensors on ``device``, uploaded once."""
        import torch

        key = str(device)
        if key not in self._dev:
            data = self.data if self.data.size else np.zeros(1, dtype=np.uint8)
            self._dev[key] = (torch.from_numpy(data).to(device), torch.from_numpy(self.offsets).to(device))
        return self._dev[key]


_FIELDS = ("guided_choice", "guided_regex", "guided_json")
_KINDS = {"guided_choice": "choice", "guided_regex": "regex", "guided_json": "json"}


def constraint_of(body: dict) -> Optional[tuple]:
    """``(kind, spec)`` of the request body's constraint, or None. More than one raises."""
    found = []
    for f in _FIELDS:
        if body.get(f) is not None:
            found.append((_KINDS[f], body[f]))
    so = body.get("structured_outputs")
    if so is not None:
        if not isinstance(so, dict):
            raise ValueError("structured_outputs must be an object")
        keys = [k for k in so if so[k] is not None]
        bad = [k for k in keys if k not in ("choice", "regex", "json")]
        if bad:
            raise ValueError(f"unsupported structured_outputs key(s) {bad}: choice, regex and json are supported")
        found += [(k, so[k]) for k in keys]
    rf = body.get("response_format")
    if rf is not None:
        if not isinstance(rf, dict):
            raise ValueError("response_format must be an object")
        typ = rf.get("type")
        if typ == "json_schema":
            js = rf.get("json_schema")
            if not isinstance(js, dict) or not isinstance(js.get("schema"), (dict, str)):
                raise ValueError("response_format json_schema needs json_schema.schema")
            found.append(("json", js["schema"]))
        elif typ not in (None, "text", "json_object"):
            raise ValueError(f"unsupported response_format type {typ!r}")
    if len(found) > 1:
        raise ValueError("at most one of guided_choice, guided_regex, guided_json, structured_outputs and "
                         "response_format json_schema may be given")
    if not found:
        return None
    kind, spec = found[0]
    if kind == "json" and isinstance(spec, str):
        try:
            spec = json.loads(spec)
        except json.JSONDecodeError as e:
            raise ValueError(f"guided_json is not valid JSON: {e}") from None
    return kind, spec


def from_request(body: dict, max_states: Optional[int] = None) -> Optional[Grammar]:
    """The compiled constraint of a request body (cached), or None; ValueError -> HTTP 400."""
    c = constraint_of(body)
    return None if c is None else compile_grammar(c[0], c[1], max_states)
