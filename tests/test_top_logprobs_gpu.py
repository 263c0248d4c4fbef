"""`ops.top_logprobs` (csrc/ops/logprobs.hip) against a CPU oracle: ids from a stable descending
sort of the values in the tested dtype (exact match), log-probabilities from a float64
log-softmax (1e-3, the sampler's bound). Real vocabulary widths, tie-heavy bf16 rows, designed
ties, masked rows, the kernel's every path, the sampler's own pick, and the engine with decode
graphs and async scheduling. Oracle and engine checks live in tests/test_top_logprobs.py."""
import pytest
import torch

from llmd_amd import ops
from llmd_amd.engine.request import SamplingParams
from test_top_logprobs import (LP_ATOL, NEG_INF, NMAX, check_against_oracle, check_greedy_invariants, run_engine,
                               tie_rows)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float32]


def _n(B, dev=DEV):
    return torch.tensor(([1, 5, 20, 0] * B)[:B], dtype=torch.int32, device=dev)


def _dev(x):
    """x on the device with 16-byte aligned rows, as the op requires: a [B, V] view of a buffer
    whose rows are padded to a multiple of 8 entries; the padding holds 1e4, so a read past V
    shows up as a wrong id."""
    B, V = x.shape
    buf = torch.full((B, -(-V // 8) * 8), 1e4, dtype=x.dtype, device=DEV)
    xd = buf[:, :V]
    xd.copy_(x)
    return xd


def _run(x_dev, n):
    ids, lp = ops.top_logprobs(x_dev, n)
    assert ids.device == x_dev.device and ids.shape == lp.shape == (x_dev.shape[0], ops.MAX_TOP_LOGPROBS)
    return ids, lp


# ---------------------------------------------------------------- random rows
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,V", [(4, 128256), (4, 151936), (5, 5003), (600, 40005)])
def test_random_rows(dtype, B, V):
    """randn * 3: bf16 rows hold fewer than V/2 distinct values (for V >= 40005), so ties sit
    at almost every cut. The last shape is a view of a wider buffer whose padding holds 1e4."""
    g = torch.Generator().manual_seed(B * 1000003 + V)
    x = (torch.randn(B, V, generator=g) * 3).to(dtype)
    if dtype == torch.bfloat16 and V >= 40005:
        assert max(len(r.unique()) for r in x[:4]) < V // 2
    xd = _dev(x)
    assert V != 40005 or (xd.stride(0) == 40008 and not xd.is_contiguous())
    n = _n(B)
    ids, lp = _run(xd, n)
    check_against_oracle(x, n.tolist(), ids, lp)


# ---------------------------------------------------------------- designed ties
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [128256, 128259])
def test_designed_ties(dtype, V):
    """Thirty 9.0s over a background below 7, n = 20: the 20 lowest of their indices, ascending.
    V = 128259 puts V-1 and V-2 into the scalar tail."""
    x, want = tie_rows(V, dtype)
    assert (x.float().sort(-1, descending=True).values[:, 30] < 7).all()
    n = torch.full((x.shape[0],), 20, dtype=torch.int32, device=DEV)
    ids, lp = _run(_dev(x), n)
    assert ids.tolist() == want
    check_against_oracle(x, n.tolist(), ids, lp)


@pytest.mark.parametrize("dtype", DTYPES)
def test_constant_and_sorted_rows(dtype):
    """Rows whose order follows the index: all equal (every cut is a tie: ids 0..n-1), ascending
    and descending ramps, and a row whose large entries all fall to one lane position of the
    kernel's workgroup, which overflows its candidate buffer and takes the round-by-round path."""
    V = 40005
    per = 8 if dtype == torch.bfloat16 else 4
    x = torch.zeros(5, V)
    x[0] = 1.5
    x[1] = torch.arange(V) / 4096.0          # ascending; bf16 rounds it into runs of equal values
    x[2] = -torch.arange(V) / 4096.0
    x[3] = -2.0
    # 16-byte chunk c goes to lane position c % 64: three positions hold every large entry
    lane3 = [i for c in range(V // per) if c % 64 in (3, 4, 5) for i in range(c * per, c * per + per)]
    x[3, lane3] = 4.0 + torch.arange(len(lane3)) % 7   # ~1900 entries above everything else
    assert len(lane3) > 1024                            # more than the kernel's candidate slots
    x[4] = NEG_INF
    x[4, lane3] = (torch.arange(len(lane3)) % 5).float()  # masked elsewhere: fewer than n lane positions live
    x = x.to(dtype)
    for nval in (20, 3):
        n = torch.full((5,), nval, dtype=torch.int32, device=DEV)
        ids, lp = _run(_dev(x), n)
        check_against_oracle(x, n.tolist(), ids, lp)
    assert ids[0, :3].tolist() == [0, 1, 2]


# ---------------------------------------------------------------- masked rows
@pytest.mark.parametrize("dtype", DTYPES)
def test_masked_rows(dtype):
    V = 5003
    x = torch.full((3, V), NEG_INF)
    keep = [0, 7, 8, 1023, 1024, 4000, V - 2, V - 1]
    x[0, keep] = torch.tensor([0.5, 3.0, 3.0, -2.0, 1.0, 3.0, -40.0, 2.0])
    x[1] = torch.randn(V, generator=torch.Generator().manual_seed(5))
    x[2, keep] = torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    x = x.to(dtype)
    n = torch.tensor([20, 0, 20], dtype=torch.int32, device=DEV)   # an n = 0 row between two live rows
    ids, lp = _run(_dev(x), n)
    assert ids[0].tolist() == [7, 8, 4000, V - 1, 1024, 0, 1023, V - 2] + [-1] * 12
    assert ids[2].tolist() == keep + [-1] * 12
    assert (ids[1] == -1).all() and (lp[1] == NEG_INF).all()
    assert (lp[0, 8:] == NEG_INF).all() and torch.isfinite(lp[0, :8]).all()
    check_against_oracle(x, n.tolist(), ids, lp)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_vocab_and_fully_masked(dtype):
    x = torch.randn(3, 16, generator=torch.Generator().manual_seed(9))
    x[2] = NEG_INF
    x = x.to(dtype)
    n = torch.full((3,), 20, dtype=torch.int32, device=DEV)
    ids, lp = _run(_dev(x), n)
    assert (ids[:2, :16] >= 0).all() and (ids[:, 16:] == -1).all() and (lp[:, 16:] == NEG_INF).all()
    assert (ids[2] == -1).all() and (lp[2] == NEG_INF).all()
    check_against_oracle(x, n.tolist(), ids, lp)


# ---------------------------------------------------------------- agreement with the sampler
@pytest.mark.parametrize("dtype", DTYPES)
def test_agrees_with_greedy_sampler(dtype):
    B, V = 8, 128256
    x = (torch.randn(B, V, generator=torch.Generator().manual_seed(11)) * 3).to(dtype).to(DEV)
    sid, slp = ops.sample(x, want_logprob=True)
    ids, lp = _run(x, torch.full((B,), 5, dtype=torch.int32, device=DEV))
    assert ids[:, 0].tolist() == sid.tolist()
    assert (lp[:, 0] - slp).abs().max().item() <= LP_ATOL


def test_binding_rejects_bad_arguments():
    x = torch.zeros(2, 64, device=DEV, dtype=torch.bfloat16)
    C = ops.native()
    ids = torch.empty(2, NMAX, dtype=torch.int32, device=DEV)
    lp = torch.empty(2, NMAX, dtype=torch.float32, device=DEV)
    n = torch.ones(2, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        C.top_logprobs(x, n[:1], ids, lp)                     # fewer counts than rows
    with pytest.raises(RuntimeError):
        C.top_logprobs(x, n, ids[:1], lp)                     # outputs too small
    with pytest.raises(RuntimeError):
        C.top_logprobs(x, n.long(), ids, lp)
    with pytest.raises(RuntimeError):
        C.top_logprobs(torch.zeros(2, 67, device=DEV, dtype=torch.bfloat16)[:, :64], n, ids, lp)  # rows not 16-B aligned
    with pytest.raises(RuntimeError):
        C.top_logprobs(x.half(), n, ids, lp)


# ---------------------------------------------------------------- engine
def test_engine_gpu_graphs_async_and_sync():
    """tiny-llama with decode graphs, two prompts in flight and one asking for nothing; async
    scheduling at its default, then off: the same tokens and the same lists."""
    kw = dict(block_size=64, num_gpu_blocks=64, max_num_batched_tokens=256, cuda_graph_max_bs=4)
    runs = []
    for async_on in (True, False):
        a, b, outs = run_engine("cuda", async_on,
                                SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True, top_logprobs=5),
                                SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True), **kw)
        check_greedy_invariants(a, b, outs, 5, 6)
        runs.append((a.output_token_ids, [[t for t, _ in top] for top in a.output_top_logprobs],
                     b.output_token_ids))
    assert runs[0] == runs[1]
