"""`ops.guided_mask` (csrc/ops/guided.hip) against its oracle `ref.guided_mask`: the set of masked
positions is exactly equal and every kept entry keeps its bits. Real vocabulary widths, the
vocabulary-split path, padded rows, both staging paths of the DFA (LDS and L2), several grammars
at different arena offsets in one batch, rows in every kind of state; the binding's argument
checks, the sampler's pick after the mask, and the engine with decode graphs and async
scheduling. Compiler, oracle and CPU engine checks live in tests/test_guided.py."""
import functools

import numpy as np
import pytest
import torch

from llmd_amd import ops
from llmd_amd.engine.request import SamplingParams
from llmd_amd.guided import compile_choice, compile_regex
from llmd_amd.ops import reference as ref
from test_guided import CHOICES, PROMPT, TOK, check_guided_output, make_engine, run, synthetic_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float32]
ALPHABET = b"0123456789-abcdef"
EOS_IDS = [2, 1001]


@functools.lru_cache(maxsize=None)
def arena():
    """Three grammars at different offsets of one arena, and eight (grammar, state) rows:
    start / mid / accepting with continuations / accepting terminal of a small grammar (LDS
    path) and of a 300-string choice trie (above the LDS threshold), and -1."""
    rng = np.random.default_rng(11)
    small = compile_regex(r"[0-9]{3}-[a-f]+")
    words = {"ab", "abc", "0-"}
    while len(words) < 300:
        words.add(bytes(rng.choice(list(ALPHABET), size=int(rng.integers(3, 11))).tolist()).decode())
    words = sorted(words)
    big = compile_choice(words)
    tiny = compile_choice(["beta", "be", "a0"])
    lds = ops.native().guided_lds_states()
    assert small.num_states <= lds and tiny.num_states <= lds < big.num_states
    cap = 8 + small.num_states + 3 + big.num_states + 5 + tiny.num_states + 2
    trans, accept = np.zeros((cap, 256), dtype=np.uint16), np.zeros(cap, dtype=np.uint8)
    trans[:8], trans[-2:] = 7, 9  # junk around the grammars: never read
    offs, o = {}, 8
    for g, gap in ((small, 3), (big, 5), (tiny, 0)):
        trans[o:o + g.num_states], accept[o:o + g.num_states] = g.trans, g.accept
        offs[g.uid] = o
        o += g.num_states + gap
    leaf = next(w for w in words if not any(v != w and v.startswith(w) for v in words))
    rows = [(small, 1), (small, small.advance(1, b"12")), (small, small.advance(1, b"123-a")),
            (tiny, tiny.advance(1, b"beta")), (None, -1),
            (big, 1), (big, big.advance(1, b"ab")), (big, big.advance(1, leaf.encode()))]
    assert small.accept[rows[2][1]] and small.trans[rows[2][1]].any()           # accepting, continues
    assert tiny.accept[rows[3][1]] and not tiny.trans[rows[3][1]].any()         # accepting, terminal
    assert big.accept[rows[6][1]] and big.trans[rows[6][1]].any() and not big.trans[rows[7][1]].any()
    assert not small.accept[rows[1][1]] and all(s != 0 for g, s in rows if g is not None)
    dev = (torch.from_numpy(trans).to(DEV), torch.from_numpy(accept).to(DEV))
    return trans, accept, dev, offs, rows


@functools.lru_cache(maxsize=None)
def table(V):
    """Synthetic token table: lengths 0, 1, 2..48 and a few of 128 bytes over the grammars'
    alphabet (so that long walks survive), two EOS ids of length 0."""
    data, off = synthetic_table(V, np.random.default_rng(V), EOS_IDS, alphabet=ALPHABET, long_tokens=4)
    lens = np.diff(off)
    assert {0, 1, 2, 48, 128} <= set(lens.tolist())
    # the 128-byte tokens of hex digits are legal somewhere: [a-f]+ keeps an all-letter one alive
    t = int(np.flatnonzero(lens == 128)[0])
    data[off[t]:off[t + 1]] = np.frombuffer(b"abcdef" * 21 + b"ab", dtype=np.uint8)
    return data, off, (torch.from_numpy(data).to(DEV), torch.from_numpy(off).to(DEV))


def _dev(x):
    """x on the device as a [B, V] view of a buffer whose rows are padded to a multiple of 8
    entries (16-byte aligned rows); the padding holds 1e4 and must stay 1e4."""
    B, V = x.shape
    buf = torch.full((B, -(-V // 8) * 8), 1e4, dtype=x.dtype, device=DEV)
    xd = buf[:, :V]
    xd.copy_(x)
    return buf, xd


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _check(x, pick, dtype):
    """Kernel == oracle on rows whose (grammar, state) are arena().rows[pick[r]]."""
    trans, accept, (d_trans, d_accept), offs, rows = arena()
    B, V = x.shape
    data, off, (d_data, d_off) = table(V)
    sel = [rows[k] for k in pick]
    dfa_off = [offs[g.uid] if g is not None else 0 for g, _ in sel]
    dfa_n = [g.num_states if g is not None else 0 for g, _ in sel]
    state = [s for _, s in sel]
    want = ref.guided_mask(x.clone(), trans, accept, dfa_off, dfa_n, state, data, off, EOS_IDS)
    buf, xd = _dev(x)
    out = ops.guided_mask(xd, d_trans, d_accept, dfa_off, dfa_n, state, d_data, d_off, EOS_IDS)
    assert out is xd
    got = xd.cpu()
    masked, want_masked = torch.isinf(got) & (got < 0), torch.isinf(want) & (want < 0)
    assert torch.equal(masked, want_masked), f"{(masked != want_masked).sum().item()} positions differ"
    assert torch.equal(_bits(got)[~masked], _bits(x)[~masked])       # kept entries: the same bits
    assert torch.equal(_bits(got), _bits(want))
    assert (buf[:, V:] == 1e4).all()                                 # nothing at index >= V is touched
    for r, (g, s) in enumerate(sel):
        if g is None:
            assert torch.equal(_bits(got[r]), _bits(x[r]))
        elif not g.trans[s].any():                                   # terminal: only the EOS ids survive
            assert (~masked[r]).nonzero().flatten().tolist() == sorted(EOS_IDS)
        else:
            assert 0 < masked[r].sum() < V
    return got


def _x(B, V, dtype):
    g = torch.Generator().manual_seed(B * 1000003 + V)
    return (torch.randn(B, V, generator=g) * 3).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,V", [(4, 128256), (4, 201088), (5, 5003), (600, 40005)])
def test_mask_matches_oracle(dtype, B, V):
    """Every row kind in one batch (B = 4: two batches, so that each kind runs at the real
    widths); the last shape is a view of a buffer padded to 40008 per row."""
    x = _x(B, V, dtype)
    if B == 4:
        _check(x, [0, 5, 2, 7], dtype)
        _check(x, [6, 4, 3, 1], dtype)
    else:
        _check(x, [r % 8 for r in range(B)], dtype)
    if V == 40005:
        assert _dev(x)[1].stride(0) == 40008


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [128256, 201088])
@pytest.mark.parametrize("kind", [0, 2, 3, 5, 6, 4])
def test_single_row_takes_the_vocabulary_split_path(dtype, V, kind):
    assert ops.native().guided_splits(1, V) > 1 and ops.native().guided_splits(600, V) == 1
    _check(_x(1, V, dtype), [kind], dtype)


def test_binding_argument_checks():
    C = ops.native()
    _, _, (tr, ac), offs, rows = arena()
    V = 5003
    _, _, (d_data, d_off) = table(V)
    g = rows[0][0]
    i32 = lambda v: torch.tensor([v, v], dtype=torch.int32, device=DEV)  # noqa: E731
    x = torch.zeros(2, 5008, device=DEV, dtype=torch.bfloat16)[:, :V]
    good = [x, tr, ac, i32(offs[g.uid]), i32(g.num_states), i32(1), d_data, d_off, EOS_IDS]
    C.guided_mask(*good)
    torch.cuda.synchronize()

    def bad(i, v):
        a = list(good)
        a[i] = v
        with pytest.raises(RuntimeError):
            C.guided_mask(*a)

    bad(0, x.half())                                                              # logits dtype
    bad(0, x.cpu())
    bad(0, torch.zeros(2, 5011, device=DEV, dtype=torch.bfloat16)[:, :V])         # rows not 16-B aligned
    bad(0, torch.zeros(2, 5009, device=DEV, dtype=torch.float32)[:, :V])
    bad(0, torch.zeros(2, 5016, device=DEV, dtype=torch.bfloat16)[:, 1:V + 1])    # base not 16-B aligned
    bad(1, tr.view(torch.int16))                                                  # trans dtype
    bad(1, tr[:, :128])
    bad(1, tr.cpu())
    bad(2, ac[: tr.shape[0] - 1])                                                 # accept shorter than the arena
    bad(2, ac.to(torch.int32))
    for i in (3, 4, 5):
        bad(i, good[i].long())                                                    # per-row dtype
        bad(i, good[i][:1])                                                       # per-row size
    bad(6, d_data.to(torch.int8))
    bad(7, d_off[:V])                                                             # offsets need V + 1 entries
    bad(7, d_off.long())
    bad(8, [V])                                                                   # EOS outside the vocabulary
    bad(8, list(range(9)))
    torch.cuda.synchronize()


def test_sampler_never_returns_a_forbidden_id():
    """64 seeded rows at temperature 1: ops.sample after the mask picks only allowed ids."""
    B, V = 64, 5003
    x = _x(B, V, torch.float32)
    pick = [r % 8 for r in range(B)]
    got = _check(x, pick, torch.float32)
    trans, accept, (d_trans, d_accept), offs, rows = arena()
    data, off, (d_data, d_off) = table(V)
    _, xd = _dev(x)
    sel = [rows[k] for k in pick]
    ops.guided_mask(xd, d_trans, d_accept, [offs[g.uid] if g else 0 for g, _ in sel],
                    [g.num_states if g else 0 for g, _ in sel], [s for _, s in sel], d_data, d_off, EOS_IDS)
    temps = torch.ones(B, device=DEV)
    for rep in range(4):
        seeds = torch.arange(B, device=DEV, dtype=torch.int64) * 7919 + rep
        ids, _ = ops.sample(xd, temps, seeds)
        for r, t in enumerate(ids.tolist()):
            assert 0 <= t < V and got[r, t] != float("-inf"), (r, t)


def test_engine_gpu_graphs_async_and_sync():
    """tiny-llama with decode graphs: a guided_regex and a guided_choice request beside a free
    one; async scheduling at its default, then off: valid outputs, the same in both modes."""
    g, gc = compile_regex(r"[0-9]{3}-[a-f]{2,6}"), compile_choice(CHOICES)
    kw = dict(device="cuda", enforce_eager=False, block_size=64, num_gpu_blocks=64, max_num_batched_tokens=256,
              cuda_graph_max_bs=4, max_num_seqs=4)
    runs = []
    for async_on in (True, False):
        eng = make_engine(async_on, **kw)
        assert eng.runner.graphs
        jobs = [(PROMPT, SamplingParams(max_tokens=16, temperature=0.0, guided=g)),
                (TOK.encode("free text"), SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True)),
                (PROMPT, SamplingParams(max_tokens=16, temperature=1.0, seed=5, guided=gc))]
        reqs, _ = run(eng, jobs)
        eng.shutdown()
        check_guided_output(reqs[0], g)
        check_guided_output(reqs[2], gc)
        assert reqs[0].finish_reason == reqs[2].finish_reason == "stop" and len(reqs[1].output_token_ids) == 12
        runs.append([r.output_token_ids for r in reqs])
    assert runs[0] == runs[1]
