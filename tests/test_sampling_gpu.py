"""The HIP sampler (Gumbel-max `ops.sample`, split / merge / scalar-tail paths) and the
3-pass radix select (`ops.topk_topp_mask`) against float64 oracles on the CPU, at real
vocabulary sizes, with ties, pre-masked rows and thresholds decided in each radix digit.
The designed rows and oracles live in tests/test_sampling_ref.py."""
import numpy as np
import pytest
import torch

from llmd_amd import ops
from llmd_amd.ops import reference as ref
from test_sampling_ref import (K_JOINT, KEEP_JOINT, NEG_INF, P_JOINT, designed_cases,
                               engine_topk_topp_cases, head_row, joint_row, p_for, run_mask, top_of_head,
                               topk_keep, topp_keep)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float32]
V_BIG = 151936


# ---------------------------------------------------------------- sampler: finite Gumbel keys
def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _seed_with_top_draw(V, seeds=range(2000)):
    """First (seed, index) whose 24-bit draw is 0xFFFFFF (numpy mirror of the kernel's hash):
    (0xFFFFFF + 0.5) / 2^24 rounds to 1.0 in fp32, which made the Gumbel key +inf."""
    with np.errstate(over="ignore"):
        inner = _mix64(np.arange(V, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15))
        for s in seeds:
            hit = np.nonzero((_mix64(np.uint64(s) ^ inner) >> np.uint64(40)) == np.uint64(0xFFFFFF))[0]
            if hit.size:
                return s, int(hit[0])
    return None


def test_sample_every_gumbel_key_finite_bf16():
    """2048 x 151936 draws: logit 40 at index 7 against 0 elsewhere loses with chance ~1e-9 over
    the whole batch, so any other id is a key that ignored its logit."""
    B = 2048
    logits = torch.zeros(B, V_BIG, device=DEV, dtype=torch.bfloat16)
    logits[:, 7] = 40.0
    temps = torch.ones(B, device=DEV)
    seeds = torch.arange(B, device=DEV, dtype=torch.int64)
    ids, lp = ops.sample(logits, temps, seeds, want_logprob=True)
    bad = (ids != 7).nonzero().flatten().tolist()
    assert not bad, f"{len(bad)} of {B} rows picked another token: rows {bad[:20]} ids {ids[bad[:20]].tolist()}"
    assert torch.isfinite(lp).all()


def test_sample_gumbel_key_finite_fp32_split():
    """One fp32 row is split over several workgroups: the affected draw goes through the merge kernel."""
    found = _seed_with_top_draw(V_BIG)
    assert found is not None, "hash mirror finds no 0xFFFFFF draw among seeds 0..1999"
    seed, idx = found
    assert idx != 7
    logits = torch.zeros(1, V_BIG, device=DEV)
    logits[0, 7] = 40.0
    ids, _ = ops.sample(logits, torch.ones(1, device=DEV), torch.tensor([seed], device=DEV, dtype=torch.int64))
    assert ids.item() == 7, f"seed {seed}: picked {ids.item()}, the mirror's 0xFFFFFF draw is index {idx}"


# ---------------------------------------------------------------- sampler: tail and split paths
V_TAIL, V_PAD = 40005, 40008          # V % 8 = 5, V % 4 = 1; rows >= 32768 entries split in two for B < 512
B_SPLIT, B_UNSPLIT = 4, 600
BIG = 9.0                             # above every randn draw


def _split_start(dtype):
    """First index of the second of two workgroups' ranges: ceil(nchunk / 2) chunks of 16 bytes."""
    w = 8 if dtype == torch.bfloat16 else 4
    return (V_TAIL // w + 1) // 2 * w


def _padded_randn(B, dtype, seed):
    """[B, V_TAIL] view of a [B, V_PAD] buffer (rows stay 16-byte aligned); the padding holds a
    value that would win every argmax if the kernel read past V."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf = torch.full((B, V_PAD), 1e4, device=DEV, dtype=dtype)
    x = buf[:, :V_TAIL]
    x.copy_(torch.randn(B, V_TAIL, device=DEV, generator=g))
    assert x.stride(0) == V_PAD and float(x.max()) < BIG - 2
    return x


def _logprob64(x, ids):
    return torch.log_softmax(x.cpu().double(), -1).gather(1, ids.cpu()[:, None]).squeeze(1)


@pytest.mark.parametrize("B", [B_SPLIT, B_UNSPLIT])
@pytest.mark.parametrize("dtype", DTYPES)
def test_sample_tail_split_greedy(dtype, B):
    x = _padded_randn(B, dtype, 1)
    places = [V_TAIL - 1, V_TAIL - 5, 0, _split_start(dtype)]
    want = torch.tensor([places[i % 4] for i in range(B)], device=DEV)
    x[torch.arange(B, device=DEV), want] = BIG
    ids, lp = ops.sample(x, want_logprob=True)
    assert torch.equal(ids, want)
    torch.testing.assert_close(lp.cpu().double(), _logprob64(x, ids), atol=1e-3, rtol=0)


@pytest.mark.parametrize("B", [B_SPLIT, B_UNSPLIT])
@pytest.mark.parametrize("dtype", DTYPES)
def test_sample_greedy_ties_lowest_index(dtype, B):
    s = _split_start(dtype)
    ties = [[s - 1, 20004, 39000],                       # one in each workgroup of a split row
            [23, 19, 16],                                # one 8-wide chunk
            [V_TAIL - 1, V_TAIL - 2, V_TAIL - 4],        # tail (fp32: last chunk and tail)
            [30000, 9000, 1000]]                         # the lower index sits in a higher thread
    x = _padded_randn(B, dtype, 2)
    for i in range(B):
        x[i, ties[i % 4]] = BIG
    want = torch.tensor([min(ties[i % 4]) for i in range(B)], device=DEV)
    ids, lp = ops.sample(x, want_logprob=True)
    assert torch.equal(ids, want)
    torch.testing.assert_close(lp.cpu().double(), _logprob64(x, ids), atol=1e-3, rtol=0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sample_tail_split_seeded_matches_unsplit(dtype):
    x = _padded_randn(B_UNSPLIT, dtype, 3)
    temps = torch.full((B_UNSPLIT,), 0.8, device=DEV)
    seeds = torch.arange(B_UNSPLIT, device=DEV, dtype=torch.int64) * 31 + 5
    ids_big, lp_big = ops.sample(x, temps, seeds, want_logprob=True)
    n = B_SPLIT
    ids_small, lp_small = ops.sample(x[:n], temps[:n], seeds[:n], want_logprob=True)
    assert torch.equal(ids_small, ids_big[:n])
    torch.testing.assert_close(lp_small, lp_big[:n], atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(lp_big.cpu().double(), _logprob64(x, ids_big), atol=1e-3, rtol=0)
    assert ids_big.unique().numel() > B_UNSPLIT // 2      # draws, not an argmax


@pytest.mark.parametrize("dtype", DTYPES)
def test_sample_distribution_masked_row_with_tail(dtype):
    n, T = 20000, 0.7
    idx = torch.tensor([0, 17, 4099, 12345, 20000, 31111, 39999, V_TAIL - 1])
    vals = torch.tensor([0.0, 1.0, 2.0, 0.5, -1.0, 0.0, 3.0, 1.5])
    row = torch.full((V_TAIL,), NEG_INF)
    row[idx] = vals
    logits = row.to(DEV, dtype).unsqueeze(0).expand(n, V_TAIL)     # stride 0: every row is the same memory
    temps = torch.full((n,), T, device=DEV)
    seeds = torch.arange(n, device=DEV, dtype=torch.int64) * 7919 + 3
    ids, lp = ops.sample(logits, temps, seeds, want_logprob=True)
    cnt = torch.bincount(ids.cpu(), minlength=V_TAIL)
    assert int(cnt[idx].sum()) == n, "a masked index was returned"
    p = torch.softmax(vals.double() / T, 0)
    assert (cnt[idx].double() / n - p).abs().max() < 0.015
    torch.testing.assert_close(lp.cpu().double(), torch.log_softmax(row.double(), 0)[ids.cpu()], atol=1e-3, rtol=0)


# ---------------------------------------------------------------- radix select
@pytest.mark.parametrize("V", [128256, V_BIG, 5003])
def test_topk_exact_with_ties(V):
    g = torch.Generator().manual_seed(V + 1)
    ks = [1, 2, 40, 1000, V - 1]
    x = (torch.randn(len(ks), V, generator=g) * 3).to(torch.bfloat16).float()
    assert not (x == 0).any()                 # the integer order puts -0 below +0
    assert all(r.unique().numel() < V // 2 for r in x)       # heavy ties, as in logits that came from bf16
    kept, _ = run_mask(ops.topk_topp_mask, list(x), ks, None, [1.0, 0.5, 2.0, 0.7, 1.3], device=DEV)
    for i, k in enumerate(ks):
        assert torch.equal(kept[i], topk_keep(x[i], k)), (V, k)


@pytest.mark.parametrize("V", [V_BIG, 5003])
def test_topk_exact_full_precision_rows(V):
    """bf16-valued rows have zero low mantissa bits, so their k-th value is settled by the first
    two radix digits; fp32 randn rows need all three."""
    g = torch.Generator().manual_seed(V + 2)
    ks = [1, 2, 40, 1000, V // 3, V - 1]
    x = torch.randn(len(ks), V, generator=g) * 3
    assert not (x == 0).any()
    kept, _ = run_mask(ops.topk_topp_mask, list(x), ks, None, [1.0, 0.5, 2.0, 0.7, 1.3, 1.0], device=DEV)
    for i, k in enumerate(ks):
        assert torch.equal(kept[i], topk_keep(x[i], k)), (V, k)
        assert int(kept[i].sum()) == k


@pytest.mark.parametrize("V", [128256, V_BIG, 5003])
def test_topp_threshold_in_each_radix_digit(V):
    cases = designed_cases(V)
    kept, _ = run_mask(ops.topk_topp_mask, [c[1] for c in cases], None, [c[5] for c in cases],
                       [c[4] for c in cases], device=DEV)
    for i, (name, row, pos, m, T, p) in enumerate(cases):
        assert torch.equal(kept[i], top_of_head(row, pos, m + 1)), (name, int(kept[i].sum()))


@pytest.mark.parametrize("V", [128256, 5003])
def test_topk_then_topp_and_premasked_rows(V):
    row, pos = joint_row(V)
    kept, _ = run_mask(ops.topk_topp_mask, [row], [K_JOINT], [P_JOINT], [1.0], device=DEV)
    assert int(kept.sum()) == KEEP_JOINT
    assert torch.equal(kept[0], top_of_head(row, pos, KEEP_JOINT))
    want, _ = run_mask(ref.topk_topp_mask, [row], [K_JOINT], [P_JOINT], [1.0])
    assert torch.equal(kept, want)
    # a row that already holds -inf (second call of the pair, min-p, logit_bias): top-p only
    row, pos = head_row(V, 3.0, 10, seed=7)
    row[::3] = NEG_INF
    assert int(torch.isfinite(row[pos]).sum()) >= 8
    p = p_for(row, 5, 1.0)
    kept, y = run_mask(ops.topk_topp_mask, [row], None, [p], [1.0], device=DEV)
    assert (y[0, ::3] == NEG_INF).all()
    assert torch.equal(kept[0], topp_keep(row, p, 1.0)) and int(kept.sum()) == 6


@pytest.mark.parametrize("k", [50, 0])
def test_topp_random_rows_properties(k):
    """fp32 accumulation order makes the exact cut unstable on random rows, so check what any
    correct nucleus has: a threshold set whose mass reaches p and is minimal, within the worst-case
    fp32 summation error over the finite terms (k * 2^-24 plus the exp error, or V * 2^-24)."""
    V, B = 128256, 8
    eps = 1e-5 if k else V * 2.0 ** -24
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, V, generator=g) * 2
    ps = [0.5, 0.9, 0.99, 0.5, 0.9, 0.99, 0.5, 0.9]
    ts = [1.0, 0.7, 1.3, 1.0, 0.7, 1.3, 0.7, 1.0]
    kept, _ = run_mask(ops.topk_topp_mask, list(x), [k] * B if k else None, ps, ts, device=DEV)
    for i in range(B):
        row = x[i].double()
        base = topk_keep(x[i], k)
        assert not (kept[i] & ~base).any()
        pr = torch.softmax(row.masked_fill(~base, NEG_INF) / ts[i], 0)
        dropped = base & ~kept[i]
        lo = row[kept[i]].min()
        assert kept[i].any() and (not dropped.any() or row[dropped].max() < lo), i
        p = float(np.float32(ps[i]))
        mass = pr[kept[i]].sum().item()
        assert mass >= p - eps, (i, mass, p)
        assert pr[kept[i] & (row > lo)].sum().item() < p + eps, (i, mass, p)


# ---------------------------------------------------------------- engine
def test_engine_topk_topp_gpu():
    engine_topk_topp_cases("cuda", block_size=64, num_gpu_blocks=64, max_num_batched_tokens=256,
                           cuda_graph_max_bs=4)
