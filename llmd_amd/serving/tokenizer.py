"""Tokenizers: HF ``tokenizers`` from a local directory, or a byte-level
fallback (no network: synthetic/random-weight deployments use the fallback).

Also provides the chat template rendering used by ``/v1/chat/completions``
and ``/v1/chat/completions/render`` (the render endpoint the router's
token-producer calls).
"""
from __future__ import annotations

import json
import os
import re
from typing import Optional

import numpy as np


def _table(toks: list) -> tuple:
    """(flat uint8 bytes, int32 offsets [len(toks) + 1]) of a list of byte strings."""
    off = np.zeros(len(toks) + 1, dtype=np.int32)
    np.cumsum([len(t) for t in toks], out=off[1:])
    return np.frombuffer(b"".join(toks), dtype=np.uint8).copy(), off


def _gpt2_unicode_to_byte() -> dict:
    """Inverse of the GPT-2 byte -> printable unicode map of ByteLevel BPE vocabularies."""
    keep = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
    chars, n = keep[:], 0
    for b in range(256):
        if b not in keep:
            keep.append(b)
            chars.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(keep, chars)}


class ByteTokenizer:
    """UTF-8 bytes -> ids [offset, offset+256); special ids below offset."""

    def __init__(self, vocab_size: int, bos_id: int = 1, eos_id: int = 2, offset: int = 3):
        self.vocab_size = vocab_size
        self.bos_token_id = bos_id
        self.eos_token_id = eos_id
        self.offset = offset if vocab_size > 259 else 0

    def encode(self, text: str, add_bos: bool = False) -> list[int]:
        ids = [b + self.offset for b in text.encode("utf-8")]
        return ([self.bos_token_id] if add_bos else []) + ids

    def decode(self, ids, skip_special: bool = True) -> str:
        bs = bytes((i - self.offset) & 0xFF for i in ids
                   if self.offset <= i < self.offset + 256 or not skip_special)
        return bs.decode("utf-8", errors="replace")

    def token_bytes(self, vocab_size: Optional[int] = None) -> tuple:
        """Token byte table for guided decoding (llmd_amd.guided.TokenTable): id ``offset + b``
        is the single byte ``b``; every other id (special, unused) has length 0."""
        V = max(vocab_size or 0, self.vocab_size)
        toks = [b""] * V
        for b in range(256):
            if self.offset + b < V:
                toks[self.offset + b] = bytes([b])
        return _table(toks)


class HFTokenizer:
    def __init__(self, path: str):
        from tokenizers import Tokenizer

        f = os.path.join(path, "tokenizer.json") if os.path.isdir(path) else path
        self.tok = Tokenizer.from_file(f)
        self.vocab_size = self.tok.get_vocab_size()
        cfgp = os.path.join(os.path.dirname(f), "tokenizer_config.json")
        self.bos_token_id = self.eos_token_id = None
        self.chat_template = None
        if os.path.exists(cfgp):
            with open(cfgp) as fh:
                c = json.load(fh)
            for k in ("bos_token", "eos_token"):
                v = c.get(k)
                if isinstance(v, dict):
                    v = v.get("content")
                if v is not None:
                    setattr(self, k + "_id", self.tok.token_to_id(v))
            self.chat_template = c.get("chat_template")

    def encode(self, text: str, add_bos: bool = False) -> list[int]:
        ids = self.tok.encode(text, add_special_tokens=False).ids
        if add_bos and self.bos_token_id is not None:
            ids = [self.bos_token_id] + ids
        return ids

    def decode(self, ids, skip_special: bool = True) -> str:
        return self.tok.decode(list(ids), skip_special_tokens=skip_special)

    def token_bytes(self, vocab_size: Optional[int] = None) -> tuple:
        """Token byte table for guided decoding: the bytes every id contributes to the decoded
        text. ByteLevel vocabularies (GPT-2 byte <-> unicode map) and ``\u2581`` / ``<0xNN>``
        byte-fallback vocabularies are understood; special and added tokens have length 0; any
        other decoder is refused (ValueError)."""
        spec = json.loads(self.tok.to_str())
        dec = spec.get("decoder") or {}
        kinds = {dec.get("type")} | {d.get("type") for d in dec.get("decoders") or []}
        added = {a["id"] for a in spec.get("added_tokens") or []}
        vocab = self.tok.get_vocab(with_added_tokens=True)
        V = max(vocab_size or 0, max(vocab.values(), default=-1) + 1)
        toks = [b""] * V
        if "ByteLevel" in kinds:
            u2b = _gpt2_unicode_to_byte()
            for s, i in vocab.items():
                if i in added:
                    continue
                try:
                    toks[i] = bytes(u2b[c] for c in s)
                except KeyError:
                    raise ValueError(f"token {i} ({s!r}) is not in the ByteLevel alphabet") from None
        elif kinds & {"ByteFallback", "Metaspace"}:
            fb = re.compile(r"<0x([0-9A-Fa-f]{2})>")
            for s, i in vocab.items():
                if i in added:
                    continue
                m = fb.fullmatch(s)
                toks[i] = bytes([int(m.group(1), 16)]) if m else s.replace("\u2581", " ").encode("utf-8")
        else:
            raise ValueError(f"guided decoding does not understand this tokenizer's decoder {sorted(map(str, kinds))}")
        return _table(toks)


def load_tokenizer(path: Optional[str], vocab_size: int, bos: int = 1, eos: int = 2):
    if path and os.path.exists(path):
        try:
            return HFTokenizer(path)
        except Exception:  # pragma: no cover - corrupt tokenizer file
            pass
    return ByteTokenizer(vocab_size, bos_id=bos if bos < 3 else 1, eos_id=eos if eos < 3 else 2)


def render_chat(messages: list[dict], add_generation_prompt: bool = True, style: str = "llama3",
                tools=None) -> str:
    """Built-in chat template of one model family (``serving/chat_template.py``)."""
    from .chat_template import BUILTIN

    return BUILTIN[style](messages, add_generation_prompt, tools)
