"""Device arena of compiled grammars for ``ops.guided_mask``.

``trans`` uint16 ``[cap, 256]`` and ``accept`` uint8 ``[cap]`` hold the DFAs one after the
other. A grammar is uploaded once per engine and reused by every request that names it;
memory is bounded by ``cap`` states (512 B + 1 B each). Grammars of live requests are pinned
(reference counted); unpinned ones are evicted least recently used first when room is needed,
and a grammar that cannot be placed even then raises ValueError.
"""
from __future__ import annotations

import torch

from .compiler import Grammar

DEFAULT_CAP = 32768  # states: 16 MiB of transitions


class GuidedArena:
    def __init__(self, device, cap: int = DEFAULT_CAP):
        self.device = torch.device(device)
        self.cap = int(cap)
        self.trans = torch.zeros(self.cap, 256, dtype=torch.uint16, device=self.device)
        self.accept = torch.zeros(self.cap, dtype=torch.uint8, device=self.device)
        self.slots: dict[int, list] = {}  # grammar uid -> [offset, states, pins, last use]
        self._clock = 0

    def _gaps(self):
        """Free (offset, size) ranges, in address order."""
        pos, out = 0, []
        for off, n, _, _ in sorted(self.slots.values()):
            if off > pos:
                out.append((pos, off - pos))
            pos = off + n
        if pos < self.cap:
            out.append((pos, self.cap - pos))
        return out

    def _place(self, n: int):
        for off, size in self._gaps():
            if size >= n:
                return off
        return None

    def acquire(self, g: Grammar) -> int:
        """Pin ``g`` (uploading it if needed) and return its arena offset."""
        self._clock += 1
        slot = self.slots.get(g.uid)
        if slot is not None:
            slot[2] += 1
            slot[3] = self._clock
            return slot[0]
        n = g.num_states
        off = self._place(n) if n <= self.cap else None
        while off is None and n <= self.cap:
            idle = [(s[3], uid) for uid, s in self.slots.items() if s[2] == 0]
            if not idle:
                break
            del self.slots[min(idle)[1]]
            off = self._place(n)
        if off is None:
            raise ValueError(f"grammar of {n} states does not fit the guided-decoding arena "
                             f"({self.cap} states, {sum(s[1] for s in self.slots.values())} in use by running requests)")
        # stream order puts the copy behind any step still reading an evicted grammar's rows
        self.trans[off:off + n].copy_(torch.from_numpy(g.trans))
        self.accept[off:off + n].copy_(torch.from_numpy(g.accept))
        self.slots[g.uid] = [off, n, 1, self._clock]
        return off

    def release(self, g: Grammar) -> None:
        slot = self.slots.get(g.uid)
        if slot is not None and slot[2] > 0:
            slot[2] -= 1

    def lookup(self, g: Grammar) -> tuple[int, int]:
        """(offset, states) of a pinned grammar."""
        slot = self.slots[g.uid]
        return slot[0], slot[1]
