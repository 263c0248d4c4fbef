"""`ops.prompt_logprobs` (csrc/ops/logprobs.hip prompt_logprobs_kernel) against the CPU oracle of
tests/test_prompt_logprobs.py: log-probability of the target from a float64 log-softmax (1e-3),
exact ranks, and alternatives equal to `ops.top_logprobs` on the same tensor bit for bit. Then the
engine: chunked prefill beside a decode batch with graphs and async scheduling, native op against
the reference op on the same device logits."""
import pytest
import torch

from llmd_amd import ops
from llmd_amd.ops import reference as ref
from test_prompt_logprobs import check_score
from test_top_logprobs import LP_ATOL, NEG_INF, NMAX, tie_rows
from test_top_logprobs_gpu import _dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float32]


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _run(x, xd, targets, n):
    """The op on xd (x's values on the device), checked against the oracle and ops.top_logprobs."""
    got = ops.prompt_logprobs(xd, _i32(targets), _i32(n))
    check_score(x, targets, n, got)
    ids, tlp = ops.top_logprobs(xd, _i32(n))
    assert torch.equal(got[2], ids) and torch.equal(got[3], tlp)
    return got


# ---------------------------------------------------------------- random rows
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,V", [(5, 5003), (4, 128256), (4, 151936), (300, 40005)])
def test_random_rows(dtype, R, V):
    """Targets at both ends, on either side of a 16-byte chunk edge, in the scalar tail (where V
    has one) and at random places; n = 0 rows beside n = 20 rows. The last shape is a view of a
    buffer padded to 40008 and filled with 1e4: a read past V shows as a wrong rank or logZ."""
    g = torch.Generator().manual_seed(R * 1000003 + V)
    x = (torch.randn(R, V, generator=g) * 3).to(dtype)
    per = 8 if dtype == torch.bfloat16 else 4
    fixed = [0, V - 1, per * 300 - 1, per * 300, V - 2]
    targets = (fixed + torch.randint(0, V, (R,), generator=g).tolist())[:R]
    n = ([20, 0, 1, 5] * R)[:R]
    xd = _dev(x)
    assert V != 40005 or (xd.stride(0) == 40008 and not xd.is_contiguous())
    _run(x, xd, targets, n)


# ---------------------------------------------------------------- designed ties
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [128256, 128259])
def test_designed_ties(dtype, V):
    """Thirty 9.0s over a background below 7: a target among them has rank 30 wherever it sits, the
    best entry below them rank 31. V = 128259 puts V-1 and V-2 into the scalar tail."""
    x, want = tie_rows(V, dtype)
    targets = [want[0][-1], want[1][0], want[2][7], want[3][19]]
    got = _run(x, _dev(x), targets, [20, 20, 0, 5])
    assert got[1].tolist() == [30] * 4
    below = [int(r.float().masked_fill(r == 9.0, NEG_INF).argmax()) for r in x]
    got = _run(x, _dev(x), below, [0, 20, 20, 1])
    assert (got[1] >= 31).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_constant_and_sorted_rows(dtype):
    """The rows of test_top_logprobs_gpu.test_constant_and_sorted_rows: all equal (rank V),
    ramps, and rows whose large entries sit at three lane positions, which overflow the
    candidate buffer and take the round-by-round path."""
    V = 40005
    per = 8 if dtype == torch.bfloat16 else 4
    x = torch.zeros(5, V)
    x[0] = 1.5
    x[1] = torch.arange(V) / 4096.0
    x[2] = -torch.arange(V) / 4096.0
    x[3] = -2.0
    lane3 = [i for c in range(V // per) if c % 64 in (3, 4, 5) for i in range(c * per, c * per + per)]
    x[3, lane3] = 4.0 + torch.arange(len(lane3)) % 7
    assert len(lane3) > 1024
    x[4] = NEG_INF
    x[4, lane3] = (torch.arange(len(lane3)) % 5).float()
    x = x.to(dtype)
    targets = [V // 2, V - 1, V - 1, lane3[6], 0]          # the last: a -inf target
    for nval in (20, 3, 0):
        got = _run(x, _dev(x), targets, [nval] * 5)
    assert got[1][0] == V and got[1][4] == V and got[0][4] == NEG_INF


# ---------------------------------------------------------------- bad and masked targets
@pytest.mark.parametrize("dtype", DTYPES)
def test_out_of_range_and_masked_targets(dtype):
    """A target outside [0, V) gives -inf / 0 and still its alternatives; the far ones would fault
    if they were dereferenced. A -inf target gives -inf / V; a fully masked row reports nothing."""
    V = 5003
    x = (torch.randn(8, V, generator=torch.Generator().manual_seed(4)) * 3).to(dtype)
    x[5, 9] = NEG_INF
    x[6] = NEG_INF
    x[7] = NEG_INF
    x[7, [3, 4000]] = torch.tensor([1.0, 2.0]).to(dtype)
    targets = [-1, V, 2**31 - 1, -2**31, V + 4, 9, 11, 4000]   # V + 4: inside the buffer's padding
    n = [20, 5, 0, 20, 1, 20, 20, 20]
    lp, rank, ids, _ = _run(x, _dev(x), targets, n)
    assert (lp[:7] == NEG_INF).all() and rank[:5].tolist() == [0] * 5
    assert rank[5] == V and rank[6] == V and (ids[6] == -1).all()
    assert rank[7] == 1 and ids[7].tolist() == [4000, 3] + [-1] * 18
    assert (ids[0] >= 0).all() and (ids[2] == -1).all()


def test_binding_rejects_bad_arguments():
    x = torch.zeros(2, 64, device=DEV, dtype=torch.bfloat16)
    C = ops.native()
    lp = torch.empty(2, dtype=torch.float32, device=DEV)
    rank = torch.empty(2, dtype=torch.int32, device=DEV)
    ids = torch.empty(2, NMAX, dtype=torch.int32, device=DEV)
    tlp = torch.empty(2, NMAX, dtype=torch.float32, device=DEV)
    t = torch.zeros(2, dtype=torch.int32, device=DEV)
    n = torch.ones(2, dtype=torch.int32, device=DEV)
    C.prompt_logprobs(x, t, n, lp, rank, ids, tlp)
    bad = [
        (x, t[:1], n, lp, rank, ids, tlp),                     # fewer targets than rows
        (x, torch.zeros(3, dtype=torch.int32, device=DEV), n, lp, rank, ids, tlp),  # more
        (x, t, n[:1], lp, rank, ids, tlp),
        (x, t.long(), n, lp, rank, ids, tlp),
        (x, t, n.long(), lp, rank, ids, tlp),
        (x, t.cpu(), n, lp, rank, ids, tlp),
        (x, t, n, lp[:1], rank, ids, tlp),
        (x, t, n, lp, rank.long(), ids, tlp),
        (x, t, n, lp, rank, ids[:1], tlp),
        (x, t, n, lp, rank, ids, tlp[:, :5]),
        (x, t, n, lp.double(), rank, ids, tlp),
        (torch.zeros(2, 67, device=DEV, dtype=torch.bfloat16)[:, :64], t, n, lp, rank, ids, tlp),  # misaligned rows
        (x.half(), t, n, lp, rank, ids, tlp),
        (x.cpu(), t, n, lp, rank, ids, tlp),
    ]
    for args in bad:
        with pytest.raises((RuntimeError, ValueError)):
            C.prompt_logprobs(*args)
    with pytest.raises(ValueError):
        ops.prompt_logprobs(x, t[:1], n)


# ---------------------------------------------------------------- engine
def _batch(eng, tag):
    """Three decoding requests, then a 67-token scored prompt beside them: a 32-token budget
    leaves it 29 tokens a step, so chunks [0,29) [29,58) [58,67). Returns the scored request and
    what every step was: (scoring rows planned, replayed a decode graph, launched over a step in flight)."""
    from test_prompt_logprobs import P49, P50, P67, scoring

    from llmd_amd.engine.request import SamplingParams

    steps = []
    plan, execute = eng.runner.plan, eng.runner.execute

    def plan_rec(so, bt):
        pl, reqs = plan(so, bt)
        steps.append(["score" in pl, pl["graph"], None, [(s.start, s.num_new_tokens) for s in so.prefills]])
        return pl, reqs

    def execute_rec(so, bt, *a, prev=None, **kw):
        out = execute(so, bt, *a, prev=prev, **kw)
        steps[-1][2] = prev is not None
        return out
    eng.runner.plan, eng.runner.execute = plan_rec, execute_rec
    try:
        dec = [eng.add_request(f"{tag}-d{i}", p[:7 + 2 * i], SamplingParams(max_tokens=12, temperature=0.0,
                                                                           ignore_eos=True))
               for i, p in enumerate((P50, P49, P67[30:]))]
        eng.step()
        eng.step()
        s = eng.add_request(f"{tag}-s", P67, scoring(5, max_tokens=3))
        while eng.has_unfinished():
            eng.step()
    finally:
        eng.runner.plan, eng.runner.execute = plan, execute
    assert all(len(d.output_token_ids) == 12 for d in dec) and len(s.output_token_ids) == 3
    return s, steps, [d.output_token_ids for d in dec]


def test_engine_gpu_native_against_reference_op(monkeypatch):
    """tiny-llama bf16 with decode graphs and async scheduling. The same batch with the kernel and
    with the reference op on the same device logits: equal ids and ranks, lp within LP_ATOL. A
    third, warm run takes no cache hit and is bit-identical to the first."""
    from test_prompt_logprobs import make_engine

    kw = dict(device="cuda", dtype="bfloat16", num_gpu_blocks=256, max_num_batched_tokens=32, enforce_eager=False,
              cuda_graph_max_bs=8)
    eng = make_engine(**kw)
    assert eng.async_sched and eng.runner.graphs
    nat, steps, dec_nat = _batch(eng, "cold")
    assert [st[3][-1] for st in steps if st[0]] == [(0, 29), (29, 29), (58, 9)]
    # scoring steps are eager and wait for the step in flight; the decode steps around them still
    # replay graphs, launched over the step before them
    assert all(not g and not over for sc, g, over, _ in steps if sc)
    rest = [st for st in steps if not st[0] and not st[3]]
    assert len(rest) >= 6 and all(g for _, g, _, _ in rest) and sum(over for _, _, over, _ in rest) >= 4
    assert nat.num_cached_tokens == 0 and nat.prompt_logprobs[0] is None and len(nat.prompt_logprobs) == 67

    warm, steps_w, dec_w = _batch(eng, "warm")
    assert warm.num_cached_tokens == 0 and eng.bm.lookup(torch.tensor(nat.prompt_token_ids).int().numpy(), 0) == 64
    assert [st[:2] + st[3:] for st in steps_w] == [st[:2] + st[3:] for st in steps]
    assert warm.prompt_logprobs == nat.prompt_logprobs and warm.output_token_ids == nat.output_token_ids
    assert dec_w == dec_nat

    calls = []

    def ref_op(logits, targets, n):
        assert logits.is_cuda and logits.dtype == torch.bfloat16
        calls.append(logits.shape[0])
        return ref.prompt_logprobs(logits, targets, n)
    monkeypatch.setattr(ops, "prompt_logprobs", ref_op)
    eng2 = make_engine(**kw)
    got, steps2, dec_ref = _batch(eng2, "cold")
    assert calls == [29, 29, 8] and [st[:2] + st[3:] for st in steps2] == [st[:2] + st[3:] for st in steps]
    assert dec_ref == dec_nat and got.output_token_ids == nat.output_token_ids
    err = 0.0
    for a, b in zip(nat.prompt_logprobs[1:], got.prompt_logprobs[1:]):
        assert a[1] == b[1] and [t for t, _ in a[2]] == [t for t, _ in b[2]] and len(a[2]) == 5
        err = max([err, abs(a[0] - b[0])] + [abs(x[1] - y[1]) for x, y in zip(a[2], b[2])])
    print(f"engine prompt_logprobs, kernel against the reference op on the same logits: max |lp| diff {err:.3e}")
    assert err <= LP_ATOL
