"""ops.paged_verify (speculative-decoding verify rows: the newest 1..8 tokens of a sequence in one
pass over its K/V, each with its own causal / window limit) vs the fp32 reference (GPU only)."""
import math

import pytest
import torch

from llmd_amd import ops
from llmd_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn
QS = (1, 2, 3, 5, 8)


def _close(a, b, atol=2e-2, rtol=2e-2):
    torch.testing.assert_close(a.float(), b.float(), atol=atol, rtol=rtol)


def _cache(nblk, Hkv, bs, D, L=1, dtype=torch.bfloat16):
    kv = torch.zeros(nblk, L, 2, Hkv, bs, D, device=DEV, dtype=dtype)
    return kv[:, 0, 0], kv[:, 0, 1]


def _paged_setup(lens, Hkv, D, bs, seed=0, fp8=False, ks=1.0, vs=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    nb_per = [(L + bs - 1) // bs for L in lens]
    total = sum(nb_per) + 3
    kc, vc = _cache(total, Hkv, bs, D, L=2, dtype=F8 if fp8 else torch.bfloat16)
    if fp8:
        kc.copy_(ref.to_cache(torch.randn(kc.shape, generator=g) * 2, F8, ks).to(DEV))
        vc.copy_(ref.to_cache(torch.randn(vc.shape, generator=g) * 2, F8, vs).to(DEV))
    else:
        kc.copy_(torch.randn(kc.shape, generator=g).to(DEV, torch.bfloat16))
        vc.copy_(torch.randn(vc.shape, generator=g).to(DEV, torch.bfloat16))
    perm = torch.randperm(total, generator=g)
    width = max(nb_per) + 2
    bt = torch.zeros(len(lens), width, dtype=torch.int32)
    o = 0
    for i, n in enumerate(nb_per):
        bt[i, :n] = perm[o: o + n].int()
        o += n
    return kc, vc, bt.to(DEV)


def _poisoned(kc, vc, bt, lens):
    """Copies of the caches with NaN in every slot no query may read: positions >= L of each
    sequence's blocks and every block no table names."""
    bs = kc.shape[2]
    live = torch.zeros(kc.shape[0], bs, dtype=torch.bool, device=DEV)
    for i, L in enumerate(lens):
        pos = torch.arange(L, device=DEV)
        live[bt[i, pos // bs].long(), pos % bs] = True
    out = []
    for c in (kc, vc):
        p = c.float()
        p = torch.where(live[:, None, :, None], p, torch.full_like(p, float("nan")))
        kv = torch.zeros(c.shape[0], 2, *c.shape[1:], device=DEV, dtype=c.dtype)  # block stride as the engine's
        kv[:, 0].copy_(p.to(c.dtype))
        out.append(kv[:, 0])
    assert out[0].float().isnan().any()
    return out


def _rows(qlens):
    qs = [0]
    for n in qlens[:-1]:
        qs.append(qs[-1] + n)
    t = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)  # noqa: E731
    return t(qs), t(qlens), sum(qlens)


# every q_len with every context: Q (the first token sees one key), 17 (drafts straddle a 16-key
# block), 66 (they straddle the 64-key tile), 130, 300, 1029
CASES = [(Q, L) for Q in QS for L in (Q, 17, 66, 130, 300, 1029) if L >= Q]


@pytest.mark.parametrize("Hq,Hkv,D", [(64, 8, 128), (32, 8, 128), (28, 4, 128), (8, 8, 64), (16, 1, 128)])
@pytest.mark.parametrize("bs", [16, 64])
def test_paged_verify(Hq, Hkv, D, bs):
    qlens = [c[0] for c in CASES]
    lens = [c[1] for c in CASES]
    kc, vc, bt = _paged_setup(lens, Hkv, D, bs)
    q_start, q_len, T = _rows(qlens)
    torch.manual_seed(1)
    q = torch.randn(T, (Hq + 2 * Hkv) * D, device=DEV, dtype=torch.bfloat16)
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    scale = 1 / math.sqrt(D)
    r = ref.paged_prefill(q, kc, vc, bt, q_start, q_len, sl, Hq, Hkv, D, scale)
    kp, vp = _poisoned(kc, vc, bt, lens)
    nmax = -(-max(lens) // 64)
    for split in [None, (64, nmax), (4096, 1)]:
        o = ops.paged_verify(q, kc, vc, bt, sl, q_start, q_len, Hq, Hkv, D, scale, split=split,
                             max_ctx=max(lens))
        # 64-key splits: L 66 / Q 5 leaves the last split fully masked for the first three tokens
        assert torch.isfinite(o.float()).all()
        _close(o, r)
        op = ops.paged_verify(q, kp, vp, bt, sl, q_start, q_len, Hq, Hkv, D, scale, split=split,
                              max_ctx=max(lens))
        assert torch.equal(o, op)  # nothing past a token's limit, or outside the table, is read


def test_paged_verify_single_rows_equal_decode():
    """q_len 1 everywhere is a decode step."""
    Hq, Hkv, D, bs = 32, 8, 128, 16
    lens = [1, 17, 66, 300]
    kc, vc, bt = _paged_setup(lens, Hkv, D, bs, seed=5)
    q_start, q_len, T = _rows([1] * len(lens))
    q = torch.randn(T, Hq * D, device=DEV, dtype=torch.bfloat16)
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    r = ref.paged_decode(q, kc, vc, bt, sl, Hq, Hkv, D, 0.09)
    for split in [None, (64, 5)]:
        _close(ops.paged_verify(q, kc, vc, bt, sl, q_start, q_len, Hq, Hkv, D, 0.09, split=split), r)


@pytest.mark.parametrize("Hq,Hkv,D", [(64, 8, 64), (32, 4, 128)])  # D 128 bf16: two passes per workgroup at Q 3
@pytest.mark.parametrize("fp8", [False, True])
def test_paged_verify_window_sinks(fp8, Hq, Hkv, D):
    """Window 128: the window start differs per token (L 131, 700), is 0 for some tokens and not for
    others (L 131 with Q 5 / 8), or is 0 for all (L 5, 128)."""
    bs = 16
    cases = [(1, 5), (3, 5), (5, 5), (2, 128), (8, 128), (2, 131), (5, 131), (8, 131), (3, 700), (8, 700)]
    qlens, lens = [c[0] for c in cases], [c[1] for c in cases]
    kc, vc, bt = _paged_setup(lens, Hkv, D, bs, seed=3, fp8=fp8)
    q_start, q_len, T = _rows(qlens)
    torch.manual_seed(2)
    q = torch.randn(T, Hq * D, device=DEV, dtype=torch.bfloat16)
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    sinks = torch.randn(Hq, device=DEV)
    kp, vp = _poisoned(kc, vc, bt, lens)
    for window in [0, 128]:
        r = ref.paged_prefill(q, kc, vc, bt, q_start, q_len, sl, Hq, Hkv, D, 0.125, window, sinks)
        for split in [None, (64, 11), (4096, 1)]:
            o = ops.paged_verify(q, kc, vc, bt, sl, q_start, q_len, Hq, Hkv, D, 0.125, window, sinks,
                                 split=split, max_ctx=700)
            assert torch.isfinite(o.float()).all()
            _close(o, r)
            op = ops.paged_verify(q, kp, vp, bt, sl, q_start, q_len, Hq, Hkv, D, 0.125, window, sinks,
                                  split=split, max_ctx=700)
            assert torch.equal(o, op)


@pytest.mark.parametrize("Hq,Hkv,D", [(64, 8, 128), (28, 4, 128), (8, 8, 64)])
def test_paged_verify_fp8(Hq, Hkv, D):
    """fp8 e4m3 cache with non-unit dequantisation scales."""
    cases = [(Q, L) for Q in QS for L in (Q, 66, 300, 1029)]
    qlens, lens = [c[0] for c in cases], [c[1] for c in cases]
    ks, vs = 0.75, 1.5
    kc, vc, bt = _paged_setup(lens, Hkv, D, 64, seed=7, fp8=True, ks=ks, vs=vs)
    q_start, q_len, T = _rows(qlens)
    torch.manual_seed(3)
    q = torch.randn(T, (Hq + 2 * Hkv) * D, device=DEV, dtype=torch.bfloat16)
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    scale = 1 / math.sqrt(D)
    r = ref.paged_prefill(q, kc, vc, bt, q_start, q_len, sl, Hq, Hkv, D, scale, k_scale=ks, v_scale=vs)
    kp, vp = _poisoned(kc, vc, bt, lens)
    for split in [None, (64, 17), (4096, 1)]:
        o = ops.paged_verify(q, kc, vc, bt, sl, q_start, q_len, Hq, Hkv, D, scale, split=split,
                             max_ctx=max(lens), k_scale=ks, v_scale=vs)
        assert torch.isfinite(o.float()).all()
        _close(o, r)
        op = ops.paged_verify(q, kp, vp, bt, sl, q_start, q_len, Hq, Hkv, D, scale, split=split,
                              max_ctx=max(lens), k_scale=ks, v_scale=vs)
        assert torch.equal(o, op)


def test_paged_verify_workspace_and_out():
    """Caller-owned workspace and output, rows offset inside a wider q (the engine's layout)."""
    Hq, Hkv, D, bs = 32, 8, 128, 16
    qlens, lens = [5, 1, 3], [300, 40, 131]
    kc, vc, bt = _paged_setup(lens, Hkv, D, bs, seed=9)
    q_start, q_len, T = _rows(qlens)
    q = torch.randn(T, (Hq + 2 * Hkv) * D, device=DEV, dtype=torch.bfloat16)
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    r = ref.paged_prefill(q, kc, vc, bt, q_start, q_len, sl, Hq, Hkv, D, 0.09)
    ws = (torch.full((T * Hq * 5 * D,), float("nan"), device=DEV),
          torch.full((T * Hq * 5 * 2,), float("nan"), device=DEV))
    out = torch.empty(T, Hq * D, device=DEV, dtype=torch.bfloat16)
    o = ops.paged_verify(q, kc, vc, bt, sl, q_start, q_len, Hq, Hkv, D, 0.09, split=(64, 5), out=out,
                         workspace=ws, max_q=5)
    assert o is out
    _close(out, r)


def test_paged_verify_refusals():
    kc, vc, bt = _paged_setup([20], 1, 128, 16)
    sl = torch.tensor([20], dtype=torch.int32, device=DEV)
    q_start, q_len, T = _rows([9])
    q = torch.randn(T, 16 * 128, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.paged_verify(q, kc, vc, bt, sl, q_start, q_len, 16, 1, 128, 0.1)
    q_start, q_len, T = _rows([2])
    q = torch.randn(T, 32 * 128, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.paged_verify(q, kc, vc, bt, sl, q_start, q_len, 32, 1, 128, 0.1)
