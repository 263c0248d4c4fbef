"""Engine step time of speculative-decoding verify steps against the plain decode step, the
break-even acceptance rate, and tokens/s / ITL at synthetic acceptance rates.

One engine per model (random-init weights), built with --speculative-config. The plain decode
step is measured on the same engine with speculation switched off at run time, which is the
state of an engine started without the flag: hipGraph replay and async scheduling. Verify steps
run eager and synchronous (graph capture of verify steps is not implemented).

Requests start the way bench.py starts them: one prompt of CTX tokens is prefilled, the others
get copies of its KV (bench._land_prompt_kv). Random weights give no natural acceptance - their
logits are near flat, and even the recorded greedy continuation of a prompt is not reproduced by
another batch shape - so acceptance is synthetic: the proposer drafts random tokens and the
step's sampled rows are rewritten on the host so that every draft position is accepted
independently with probability p (the forward pass, the sampler and the scheduler's acceptance
run unchanged; only the token values differ, and the cost of a step does not depend on them).
With that model a verify step emits E(p, k) = (1 - p^(k+1)) / (1 - p) tokens per request, and
speculation breaks even where E(p, k) = t_verify / t_decode.

Also timed: the host cost of the n-gram proposer (index build, and append + propose per step)
for 64 requests at a 5000-token context.
  python scripts/bench_spec_decode.py [--models llama-3-8b,llama-3-70b] [--ctx 5000] [--batches 1,8,64]
      [--ks 2,4] [--steps 30] [--warmup 10] [--device cuda]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import _land_prompt_kv  # noqa: E402
from llmd_amd.engine.config import EngineConfig  # noqa: E402
from llmd_amd.engine.engine import LLMEngine  # noqa: E402
from llmd_amd.engine.request import Request, SamplingParams  # noqa: E402
from llmd_amd.engine.spec_decode import NgramProposer, SpeculativeConfig  # noqa: E402


def sync(dev):
    if dev == "cuda":
        torch.cuda.synchronize()


def expected_tokens(p, k):
    return k + 1.0 if p >= 1.0 else (1 - p ** (k + 1)) / (1 - p)


def break_even(ratio, k):
    """p with E(p, k) = ratio (t_verify / t_decode), or None when even p = 1 does not reach it."""
    if ratio <= 1.0:
        return 0.0
    if ratio >= k + 1:
        return None
    lo, hi = 0.0, 1.0
    for _ in range(50):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if expected_tokens(mid, k) < ratio else (lo, mid)
    return hi


class Bench:
    def __init__(self, model, a):
        self.a, self.dev = a, a.device
        kmax = max(a.ks)
        self.max_out = (kmax + 1) * (a.warmup + a.steps) + 8
        cfg = EngineConfig.create(
            model, device=a.device, block_size=a.block_size, max_num_seqs=max(a.batches) + 1,
            max_num_batched_tokens=8192, max_model_len=a.ctx + self.max_out + 64, enable_prefix_caching=True,
            cuda_graph_max_bs=max(a.batches), async_scheduling=True,
            speculative_config={"method": "ngram", "num_speculative_tokens": kmax})
        t0 = time.time()
        self.eng = LLMEngine(cfg)
        sync(self.dev)
        self.vocab = cfg.model_config.vocab_size
        print(f"# {model}: engine up in {time.time() - t0:.0f}s, {self.eng.runner.num_blocks} KV blocks", flush=True)
        self.spec = self.eng.spec
        self.prompt = np.random.default_rng(1).integers(100, self.vocab - 100, size=a.ctx).tolist()
        self.n = 0
        # the source of every other request's prompt KV: prefilled once, then parked (it keeps its blocks)
        self.speculate(False)
        self.src = self.add(1 << 20)
        while self.src.num_computed_tokens < a.ctx:
            self.eng.step()
        self.eng.drain()
        sync(self.dev)
        self.eng.sched.running.remove(self.src)
        self.accept_p, self.rng = 0.0, np.random.default_rng(0)
        real = self.eng.runner.execute

        def execute(so, bt, **kw):  # synthetic acceptance: see the module docstring
            sampled = real(so, bt, **kw)
            for sr in so.verifies:
                rows = list(sampled[sr.req.seq_id])
                for j, d in enumerate(sr.drafts):
                    if self.rng.random() < self.accept_p:
                        rows[j] = (d, rows[j][1])
                    else:
                        if rows[j][0] == d:
                            rows[j] = ((d + 1) % self.vocab, rows[j][1])
                        break
                sampled[sr.req.seq_id] = rows
            return sampled
        self.eng.runner.execute = execute

    def speculate(self, on, k=None):
        e = self.eng
        e.drain()
        e.spec = e.sched.spec = self.spec if on else None
        e.async_sched = not on
        if on:
            self.spec.k = k

    def add(self, max_tokens):
        self.n += 1
        return self.eng.add_request(f"r{self.n}", self.prompt,
                                    SamplingParams(max_tokens=max_tokens, temperature=0.0, ignore_eos=True))

    def batch(self, B):
        reqs = [self.add(self.max_out) for _ in range(B)]
        landed = sum(_land_prompt_kv(self.eng, r, self.src) for r in reqs)
        assert landed == B, f"only {landed} of {B} prompts landed as KV copies"
        sync(self.dev)
        return reqs

    def clear(self, reqs):
        self.eng.drain()
        for r in reqs:
            self.eng.abort(r.request_id)
        assert not self.eng.sched.running and not self.eng.sched.num_waiting

    def run(self, reqs, warmup, steps):
        """(seconds per step, tokens emitted per step) over `steps` steps after `warmup`."""
        for _ in range(warmup):
            self.eng.step()
        self.eng.drain()
        sync(self.dev)
        n0 = sum(len(r.output_token_ids) for r in reqs)
        t0 = time.perf_counter()
        for _ in range(steps):
            self.eng.step()
        self.eng.drain()
        sync(self.dev)
        dt = time.perf_counter() - t0
        return dt / steps, (sum(len(r.output_token_ids) for r in reqs) - n0) / steps

    def measure(self, B):
        a = self.a
        self.speculate(False)  # plain decode: graphs + async scheduling
        reqs = self.batch(B)
        t_dec, tok = self.run(reqs, a.warmup, a.steps)
        self.clear(reqs)
        print(f"batch {B:3d} plain decode (graph, async): {t_dec * 1e3:8.2f} ms/step, {tok / t_dec:9.1f} tok/s, "
              f"ITL {t_dec * 1e3:7.2f} ms", flush=True)
        for k in a.ks:
            rows = []
            for p in a.accept:
                self.speculate(True, k)
                self.accept_p = p
                self.spec.proposer = lambda r, kk: self.rng.integers(100, self.vocab - 100, kk).tolist()
                reqs = self.batch(B)
                d0, t0_, a0 = self.spec.num_drafts, self.spec.num_draft_tokens, self.spec.num_accepted_tokens
                t_ver, tok = self.run(reqs, a.warmup, a.steps)
                nd, nt, na = (self.spec.num_drafts - d0, self.spec.num_draft_tokens - t0_,
                              self.spec.num_accepted_tokens - a0)
                self.clear(reqs)
                rows.append((p, t_ver, tok, na / max(nt, 1), nd))
            t_ver = float(np.median([r[1] for r in rows]))
            be = break_even(t_ver / t_dec, k)
            print(f"batch {B:3d} k={k} verify step (eager, sync): {t_ver * 1e3:8.2f} ms/step = x{t_ver / t_dec:4.2f} of "
                  f"the decode step; break-even acceptance "
                  f"{'not reachable' if be is None else format(be, '.2f')}", flush=True)
            for p, tv, tok, acc, nd in rows:
                per_req = tok / B
                print(f"    p={p:.1f}: {tv * 1e3:8.2f} ms/step, accepted {acc:4.2f} of draft tokens, "
                      f"{per_req:4.2f} tok/step/request (model {expected_tokens(p, k):4.2f}), {tok / tv:9.1f} tok/s "
                      f"(x{tok / tv / (B / t_dec):4.2f} of plain), ITL {tv / max(per_req, 1e-9) * 1e3:7.2f} ms", flush=True)


def host_cost(ctx, nreq=64, steps=50):
    sc = SpeculativeConfig("ngram", 4, 4, 2)
    rng = np.random.default_rng(0)
    prop = NgramProposer(sc)
    reqs = [Request(f"h{i}", rng.integers(0, 128000, ctx).tolist(), SamplingParams()) for i in range(nreq)]
    for r in reqs:
        r.output_token_ids = [1]
    t0 = time.perf_counter()
    for r in reqs:
        prop(r, 4)
    build = time.perf_counter() - t0
    t0 = time.perf_counter()
    for _ in range(steps):
        for r in reqs:
            r.output_token_ids += r.prompt_token_ids[7:10]  # three new tokens that repeat an earlier run
            prop(r, 4)
    per = (time.perf_counter() - t0) / steps
    print(f"# n-gram proposer host cost, {nreq} requests x ctx {ctx}: index build {build * 1e3:.1f} ms once "
          f"({build / nreq * 1e3:.2f} ms/request), append + propose {per * 1e3:.3f} ms/step "
          f"({per / nreq * 1e6:.1f} us/request)", flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--models", default="llama-3-8b,llama-3-70b")
    p.add_argument("--ctx", type=int, default=5000)
    p.add_argument("--batches", default="1,8,64")
    p.add_argument("--ks", default="2,4")
    p.add_argument("--accept", default="0.3,0.6,0.9")
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--block-size", type=int, default=64)
    p.add_argument("--device", default="cuda")
    a = p.parse_args()
    a.batches = [int(x) for x in a.batches.split(",")]
    a.ks = [int(x) for x in a.ks.split(",")]
    a.accept = [float(x) for x in a.accept.split(",")]
    if a.device == "cuda" and not torch.cuda.is_available():
        sys.exit("bench_spec_decode: no GPU (a timing needs one; --device cpu only rehearses the logic)")
    models = a.models.split(",")
    if len(models) > 1:  # one process per model: the pool and the weights of the last one are gone
        host_cost(a.ctx)
        for m in models:
            argv = ["--models", m, "--ctx", str(a.ctx), "--batches", ",".join(map(str, a.batches)),
                    "--ks", ",".join(map(str, a.ks)), "--accept", ",".join(map(str, a.accept)),
                    "--steps", str(a.steps), "--warmup", str(a.warmup), "--block-size", str(a.block_size),
                    "--device", a.device]
            rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv).returncode
            if rc:
                sys.exit(rc)
        return
    for model in models:
        b = Bench(model, a)
        print(f"# {model}, ctx {a.ctx}, {a.warmup} warm-up + {a.steps} timed steps per figure; weights and "
              f"prompts random, acceptance synthetic", flush=True)
        for B in a.batches:
            b.measure(B)


if __name__ == "__main__":
    main()
