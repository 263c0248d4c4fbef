"""Top-k / top-p reference (``reference.topk_topp_mask``) against a float64 oracle, and
the engine's top-k / top-p path on the CPU.

The designed rows and oracles below are shared with tests/test_sampling_gpu.py, which
runs the same cases through the HIP radix select.

Semantics (vLLM): top-k first, then top-p over what is left, i.e. the top-p mass is
renormalised over the top-k survivors. A set of tied values is kept or dropped whole.
"""
import numpy as np
import torch

from llmd_amd.ops import reference as ref

NEG_INF = float("-inf")
HEAD_N = 24                       # entries of a designed row that carry all the mass
HEAD_M = (1, 7, 12, 23)           # keep the top m + 1 of them
QUARTER_N = 16
QUARTER_M = (1, 4, 8)
MARGIN = 1e-3                     # least distance of p to the cumulative masses next to it


# ---------------------------------------------------------------- float64 oracles
def topk_keep(row: torch.Tensor, k: int) -> torch.Tensor:
    """row >= (k-th largest value): integer logic, ties with the k-th value are kept."""
    V = row.numel()
    if not 0 < k < V:
        return torch.ones(V, dtype=torch.bool)
    kth = torch.sort(row, descending=True).values[k - 1]
    return row >= kth


def cum_mass(row: torch.Tensor, T: float):
    """Values of the finite entries in descending order and their float64 cumulative softmax mass."""
    v = torch.sort(row[torch.isfinite(row)].double(), descending=True).values
    pr = torch.softmax(v / T, 0)
    return v, torch.cumsum(pr, 0)


def topp_keep(row: torch.Tensor, p: float, T: float) -> torch.Tensor:
    """Smallest set of largest entries whose float64 mass reaches p (over the finite entries)."""
    v, cum = cum_mass(row, T)
    n = min(int((cum < p).sum()) + 1, v.numel())
    return row.double() >= v[n - 1]


def p_for(row: torch.Tensor, m: int, T: float) -> float:
    """A float32 p halfway between the mass of the top m and of the top m + 1 finite entries, so
    that top-p keeps exactly m + 1 of them; both neighbours are at least MARGIN away (the HIP
    kernel sums ~24 fp32 terms, error a few 2^-21, so the kept set is unambiguous)."""
    _, cum = cum_mass(row, T)
    p = float(np.float32((cum[m - 1].item() + cum[m].item()) / 2))
    assert p - cum[m - 1].item() >= MARGIN and cum[m].item() - p >= MARGIN, (m, T, p, cum[m - 1:m + 1])
    return p


# ---------------------------------------------------------------- designed rows
def head_values(base: float, s: int, n: int = HEAD_N) -> np.ndarray:
    """n floats whose integer images are image(base) + (j << s): s = 0 differs only in the low
    10 bits (last radix digit), s = 10 only in bits 10..20 (middle digit)."""
    img = np.array([base], dtype=np.float32).view(np.int32)[0]
    return (img + (np.arange(n, dtype=np.int32) << s)).astype(np.int32).view(np.float32)


def designed_row(V: int, vals: np.ndarray, tail_mean: float, seed: int):
    """fp32 row: `vals` at random positions, everything else tail_mean + 0.5 randn (negligible mass)."""
    g = torch.Generator().manual_seed(seed)
    row = tail_mean + 0.5 * torch.randn(V, generator=g)
    pos = torch.randperm(V, generator=g)[:len(vals)]
    row[pos] = torch.from_numpy(np.ascontiguousarray(vals))
    assert len(set(vals.tolist())) == len(vals) and float(row.max()) == float(vals.max())
    return row, pos


def head_row(V: int, base: float, s: int, seed: int = 0):
    return designed_row(V, head_values(base, s), -30.0 if base > 0 else -40.0, seed)


def quarter_row(V: int, seed: int = 0):
    """Head 4.0 - 0.25 j: neighbours differ in the top radix digit or the first bit below it."""
    return designed_row(V, (4.0 - 0.25 * np.arange(QUARTER_N)).astype(np.float32), -30.0, seed)


def designed_cases(V: int):
    """(name, row, head positions, m, T, p): top-p must keep exactly the top m + 1 head entries."""
    out = []
    rows = [(f"s{s}{'+' if base > 0 else '-'}", *head_row(V, base, s, seed=11 + s + (base < 0)), HEAD_M)
            for s in (0, 10) for base in (3.0, -3.0)]
    rows.append(("quarter", *quarter_row(V, seed=31), QUARTER_M))
    for name, row, pos, ms in rows:
        for T in (1.0, 0.5, 2.0):
            for m in ms:
                out.append((f"{name}-T{T}-m{m}", row, pos, m, T, p_for(row, m, T)))
    return out


def top_of_head(row: torch.Tensor, pos: torch.Tensor, n: int) -> torch.Tensor:
    keep = torch.zeros(row.numel(), dtype=torch.bool)
    keep[pos[torch.argsort(row[pos], descending=True)[:n]]] = True
    return keep


def run_mask(fn, rows, topk=None, topp=None, temps=None, device="cpu"):
    """fn(logits, topk, topp, temps) on a stack of fp32 rows; returns the kept mask and the output."""
    x = torch.stack(rows).float().to(device)
    k = None if topk is None else torch.tensor(topk, dtype=torch.int32, device=device)
    p = None if topp is None else torch.tensor(topp, dtype=torch.float32, device=device)
    t = None if temps is None else torch.tensor(temps, dtype=torch.float32, device=device)
    y = fn(x.clone(), k, p, t).cpu()
    kept = y != NEG_INF
    assert torch.equal(y[kept], x.cpu()[kept]), "kept logits must be unchanged"
    return kept, y


K_JOINT, P_JOINT, KEEP_JOINT = 10, 0.55, 6


def joint_row(V: int = 5003):
    """24 nearly equal head entries: top-k 10 then top-p 0.55 keeps 6 (0.6 >= 0.55 > 0.5 of the
    renormalised mass); top-p over the whole row intersected with top-k would keep 10."""
    row, pos = head_row(V, 3.0, 10, seed=5)
    _, cum = cum_mass(torch.where(topk_keep(row, K_JOINT), row, torch.full_like(row, NEG_INF)), 1.0)
    assert cum[KEEP_JOINT - 2] < P_JOINT - 0.04 and cum[KEEP_JOINT - 1] > P_JOINT + 0.04
    return row, pos


# ---------------------------------------------------------------- reference tests
def test_ref_topk_then_topp_designed_row():
    row, pos = joint_row()
    kept, _ = run_mask(ref.topk_topp_mask, [row], [K_JOINT], [P_JOINT], [1.0])
    assert int(kept.sum()) == KEEP_JOINT
    assert torch.equal(kept[0], top_of_head(row, pos, KEEP_JOINT))


def test_ref_joint_equals_sequential():
    torch.manual_seed(3)
    V = 4096
    x = torch.randn(4, V) * 2
    ks, ps, ts = [20, 50, 5, 200], [0.9, 0.8, 0.95, 0.5], [1.0, 0.7, 1.3, 1.0]
    rows = list(x) + [joint_row(V)[0]]
    ks, ps, ts = ks + [K_JOINT], ps + [P_JOINT], ts + [1.0]
    joint, _ = run_mask(ref.topk_topp_mask, rows, ks, ps, ts)
    _, after_k = run_mask(ref.topk_topp_mask, rows, ks, None, ts)
    seq, _ = run_mask(ref.topk_topp_mask, list(after_k), None, ps, ts)
    assert torch.equal(joint, seq)
    for i, row in enumerate(rows):   # and both equal the float64 oracle applied in sequence
        kk = topk_keep(row, ks[i])
        want = kk & topp_keep(torch.where(kk, row, torch.full_like(row, NEG_INF)), float(np.float32(ps[i])), ts[i])
        assert torch.equal(joint[i], want), i
    assert int(joint[-1].sum()) == KEEP_JOINT


def test_ref_topp_designed_rows():
    cases = designed_cases(5003)
    kept, _ = run_mask(ref.topk_topp_mask, [c[1] for c in cases], None, [c[5] for c in cases], [c[4] for c in cases])
    for i, (name, row, pos, m, T, p) in enumerate(cases):
        assert torch.equal(topp_keep(row, p, T), top_of_head(row, pos, m + 1)), name   # oracle vs design
        assert torch.equal(kept[i], top_of_head(row, pos, m + 1)), name


def test_ref_topp_premasked_row():
    row, pos = head_row(5003, 3.0, 10, seed=7)
    row[::3] = NEG_INF
    assert int(torch.isfinite(row[pos]).sum()) >= 8
    p = p_for(row, 5, 1.0)
    kept, y = run_mask(ref.topk_topp_mask, [row], None, [p], [1.0])
    assert (y[0, ::3] == NEG_INF).all()
    assert torch.equal(kept[0], topp_keep(row, p, 1.0)) and int(kept.sum()) == 6


# ---------------------------------------------------------------- engine
def engine_topk_topp_cases(device: str, **kw):
    """top_k = 1 and top_p -> 0 leave one candidate, so a sampled request must reproduce the greedy
    output token for token; top-k with top-p and logprobs must give finite log-probs."""
    from llmd_amd.engine.config import EngineConfig
    from llmd_amd.engine.engine import LLMEngine
    from llmd_amd.engine.request import SamplingParams

    eng = LLMEngine(EngineConfig.create("tiny-llama", device=device, max_num_seqs=4, max_model_len=256,
                                        enable_prefix_caching=False, **kw))
    prompt = np.random.default_rng(0).integers(3, 500, size=20).tolist()
    n = 6

    def run(**sp):
        r = eng.generate([prompt], SamplingParams(max_tokens=n, ignore_eos=True, **sp))[0]
        assert len(r.output_token_ids) == n
        return r

    greedy = run(temperature=0.0).output_token_ids
    assert run(temperature=1.0, seed=1, top_k=1).output_token_ids == greedy
    assert run(temperature=1.0, seed=1, top_p=1e-6).output_token_ids == greedy
    r = run(temperature=1.0, seed=1, top_k=5, top_p=0.9, logprobs=1)
    assert len(r.output_logprobs) == n and all(np.isfinite(x) and x <= 1e-6 for x in r.output_logprobs)
    assert all(0 <= t < 512 for t in r.output_token_ids)


def test_engine_topk_topp_cpu():
    engine_topk_topp_cases("cpu", block_size=16, num_gpu_blocks=64, max_num_batched_tokens=64, enforce_eager=True)
