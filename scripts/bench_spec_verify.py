"""ops.paged_verify (speculative-decoding verify rows: Q newest tokens of each sequence in one
pass over its K/V) against the two things decode attention could do before it:
  (a) ops.paged_decode on the same batch, one row per sequence: the same K/V bytes - the floor;
  (b) ops.paged_decode with the Q x B rows as separate sequences sharing block tables - what a
      step of Q x B decode rows costs (K/V read Q times).
Shapes: Llama-3-70B TP1 heads (64 q / 8 kv, D 128) and gpt-oss heads (64 / 8, D 64, attention
sinks; full layers and window-128 layers), batch 64, context 5000, block 64, bf16 and fp8 KV.
The three are timed alternately, REPS rounds of ITERS calls between device events; the median
round is reported with the spread, the achieved TB/s of the K/V bytes one pass needs, and the
ratios. Gate (exit status 1): paged_verify beats (b) at every Q >= 2.
  python scripts/bench_spec_verify.py   [SV_BATCH=64 SV_CTX=5000 SV_REPS=5 SV_ITERS=20]"""
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmd_amd import ops  # noqa: E402
from llmd_amd.ops import reference as ref  # noqa: E402

F8 = torch.float8_e4m3fn


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def main():
    B = int(os.environ.get("SV_BATCH", "64"))
    ctx = int(os.environ.get("SV_CTX", "5000"))
    reps = int(os.environ.get("SV_REPS", "5"))
    iters = int(os.environ.get("SV_ITERS", "20"))
    Hq, Hkv, bs, dev = 64, 8, 64, "cuda"
    G = Hq // Hkv
    ok = True
    print(f"batch {B} ctx {ctx} block {bs} Hq {Hq} Hkv {Hkv}; {reps} rounds x {iters} calls, median (min-max) us",
          flush=True)
    for name, D, window, sinks_on in (("70B D128", 128, 0, False), ("gpt-oss D64 full+sinks", 64, 0, True),
                                      ("gpt-oss D64 window128+sinks", 64, 128, True)):
        per = math.ceil(ctx / bs)
        nb = B * per + 1
        for fp8 in (False, True):
            g = torch.Generator(device=dev).manual_seed(0)
            kc = torch.randn(nb, Hkv, bs, D, device=dev, dtype=torch.bfloat16, generator=g)
            vc = torch.randn(nb, Hkv, bs, D, device=dev, dtype=torch.bfloat16, generator=g)
            if fp8:
                kc, vc = ref.to_cache(kc, F8, 1.0), ref.to_cache(vc, F8, 1.0)
            bt = torch.randperm(nb - 1, device=dev, generator=g)[:B * per].view(B, per).int()
            sinks = torch.randn(Hq, device=dev, generator=g) if sinks_on else None
            scale = D ** -0.5
            for Q in (1, 2, 3, 5, 8):
                T = Q * B
                q = torch.randn(T, Hq * D, device=dev, dtype=torch.bfloat16, generator=g)
                sl = torch.full((B,), ctx, dtype=torch.int32, device=dev)
                qs = (torch.arange(B, device=dev, dtype=torch.int32) * Q)
                ql = torch.full((B,), Q, dtype=torch.int32, device=dev)
                # (b): row b * Q + j is sequence b at context ctx - (Q - 1) + j
                bt_b = bt.repeat_interleave(Q, 0).contiguous()
                sl_b = (ctx - (Q - 1) + torch.arange(Q, device=dev, dtype=torch.int32)).repeat(B)
                out_v = torch.empty(T, Hq * D, device=dev, dtype=torch.bfloat16)
                out_a = torch.empty(B, Hq * D, device=dev, dtype=torch.bfloat16)
                out_b = torch.empty(T, Hq * D, device=dev, dtype=torch.bfloat16)
                eff = min(ctx, window) if window else ctx
                sp_v = ops.verify_split_plan(ctx, B, Hkv, G, Q, window, D, fp8)
                sp_a = ops.decode_split_plan(eff, B, Hkv, G)
                sp_b = ops.decode_split_plan(eff, T, Hkv, G)

                def ws(rows, split):
                    return (torch.empty(rows * Hq * split[1] * D, dtype=torch.float32, device=dev),
                            torch.empty(rows * Hq * split[1] * 2, dtype=torch.float32, device=dev))
                ws_v, ws_a, ws_b = ws(T, sp_v), ws(B, sp_a), ws(T, sp_b)
                fv = lambda: ops.paged_verify(q, kc, vc, bt, sl, qs, ql, Hq, Hkv, D, scale, window, sinks,  # noqa: E731
                                              split=sp_v, out=out_v, workspace=ws_v, max_q=Q)
                fa = lambda: ops.paged_decode(q[:B], kc, vc, bt, sl, Hq, Hkv, D, scale, window, sinks,  # noqa: E731
                                              split=sp_a, out=out_a, workspace=ws_a)
                fb = lambda: ops.paged_decode(q, kc, vc, bt_b, sl_b, Hq, Hkv, D, scale, window, sinks,  # noqa: E731
                                              split=sp_b, out=out_b, workspace=ws_b)
                for f in (fv, fa, fb):
                    for _ in range(3):
                        f()
                torch.cuda.synchronize()
                # the same rows, computed both ways, agree
                err = (out_v.float() - out_b.float()).abs().max().item()
                tv, ta, tb = [], [], []
                for _ in range(reps):
                    tv.append(timed(fv, iters))
                    ta.append(timed(fa, iters))
                    tb.append(timed(fb, iters))
                mv, ma, mb = (statistics.median(t) for t in (tv, ta, tb))
                keys = min(ctx, window + Q - 1) if window else ctx
                by = B * keys * Hkv * D * 2 * (1 if fp8 else 2)
                gate = "" if Q == 1 else ("  PASS" if mv < mb else "  FAIL")
                ok = ok and (Q == 1 or mv < mb)
                print(f"{name:28s} {'fp8 ' if fp8 else 'bf16'} Q={Q}: verify {mv:7.1f} ({min(tv):.1f}-{max(tv):.1f}) "
                      f"split {sp_v} {by / mv / 1e6:5.2f} TB/s | (a) decode B rows {ma:7.1f} ({min(ta):.1f}-{max(ta):.1f}) "
                      f"x{mv / ma:4.2f} | (b) decode QxB rows {mb:7.1f} ({min(tb):.1f}-{max(tb):.1f}) x{mv / mb:4.2f}"
                      f" | max|v-b| {err:.3g}{gate}", flush=True)
            del kc, vc
    print("gate (verify faster than (b) at every Q >= 2):", "PASS" if ok else "FAIL", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
