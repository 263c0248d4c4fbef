"""Cost of prompt scoring (ops.prompt_logprobs, csrc/ops/logprobs.hip) on one GPU.

Kernel: R = 256 bf16 rows, V = 128256 and 151936, n = 0 / 1 / 20 alternatives, against the PyTorch
composition it replaces on the same tensor (log_softmax + gather + (x >= t).sum + topk), the two
alternating window by window; median of WINDOWS device-event windows of PER launches, after a
warm-up, REPEATS times. GB/s is the row bytes (R x V x 2) over the kernel's time: the bytes one
pass needs, so a kernel that reads the rows twice (n > 0) shows about half its real traffic.

End to end: Llama-3-8B shape, random weights, one 5000-token prompt on an idle engine; time from
add_request to the first token with prompt_logprobs None (the unscored path), 0 and 1, the three
alternating, every prompt fresh. Then, on the same engine's LM head, what the 4999 scoring rows
cost in isolation in slices of LLMD_SCORE_ROWS: the logits GEMM and the kernel.
  python scripts/bench_prompt_logprobs.py [out.txt] [--kernel-only]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmd_amd import ops  # noqa: E402

R, WINDOWS, PER, REPEATS = 256, 25, 10, 2
ISL, TTFT_RUNS = 5000, 5


def window(fn, per=PER):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(per):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / per  # us per call


def torch_composition(x, t, n):
    lf = torch.log_softmax(x.float(), -1)
    lp = lf.gather(-1, t[:, None])
    rank = (x >= x.gather(-1, t[:, None])).sum(-1)
    return (lp, rank) + (tuple(lf.topk(n)) if n else ())


def kernel_table(lines):
    lines.append(f"# kernel: R={R} bf16 randn*3; us per call, median of {WINDOWS} windows x {PER} launches, "
                 f"kernel and torch alternating; {REPEATS} repeats of every row")
    slower = []
    for V in (128256, 151936):
        x = (torch.randn(R, V, generator=torch.Generator().manual_seed(V)) * 3).to(torch.bfloat16).cuda()
        t = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(1)).cuda()
        t32 = t.int()
        for n in (0, 1, 20):
            nn = torch.full((R,), n, dtype=torch.int32, device="cuda")
            fns = {"kernel": lambda: ops.prompt_logprobs(x, t32, nn), "torch": lambda: torch_composition(x, t, n)}
            got, want = fns["kernel"](), fns["torch"]()
            assert (got[0] - want[0].squeeze(-1)).abs().max().item() < 1e-3 and torch.equal(got[1].long(), want[1])
            for rep in range(REPEATS):
                for fn in fns.values():
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                ts = {k: [] for k in fns}
                for _ in range(WINDOWS):
                    for k, fn in fns.items():
                        ts[k].append(window(fn))
                med = {k: statistics.median(v) for k, v in ts.items()}
                gbs = R * V * 2 / (med["kernel"] * 1e-6) / 1e9
                lines.append(f"V={V} n={n:2d} rep{rep}: " + "  ".join(
                    f"{k} {med[k]:7.1f} (min {min(ts[k]):6.1f} max {max(ts[k]):6.1f})" for k in fns)
                    + f"  torch/kernel {med['torch'] / med['kernel']:.2f}x  row bytes / kernel time {gbs:6.0f} GB/s")
                if med["kernel"] > med["torch"]:
                    slower.append((V, n))
    lines.append(f"# gate (kernel not slower than the torch composition at any point): "
                 f"{'held' if not slower else 'MISSED at ' + str(slower)}")


def end_to_end(lines):
    from llmd_amd.engine.config import EngineConfig
    from llmd_amd.engine.engine import LLMEngine
    from llmd_amd.engine.request import SamplingParams

    cfg = EngineConfig.create("llama-3-8b", device="cuda", block_size=64, max_num_seqs=8, max_num_batched_tokens=8192,
                              max_model_len=ISL + 64, enable_prefix_caching=True, cuda_graph_max_bs=8)
    eng = LLMEngine(cfg)
    V = cfg.model_config.vocab_size
    lines.append(f"# end to end: {cfg.model_config.name} shape, random weights, V={V}, one {ISL}-token prompt, idle engine, "
                 f"max_num_batched_tokens 8192 (one chunk); num_gpu_blocks {eng.runner.num_blocks} x 64 "
                 f"(profile_and_allocate is untouched: an engine that scores nothing allocates what it did)")
    rng = np.random.default_rng(0)
    ttft = {None: [], 0: [], 1: []}

    def once(n, k):
        toks = rng.integers(100, V - 100, size=ISL).tolist()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = eng.add_request(f"r{k}", toks, SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True,
                                                          prompt_logprobs=n))
        while eng.has_unfinished():
            eng.step()
        dt = time.perf_counter() - t0
        assert len(r.output_token_ids) == 1 and (n is None or r.prompt_logprobs[-1] is not None)
        return dt * 1e3

    for n in ttft:  # warm-up of every path
        once(n, f"w{n}")
    for k in range(TTFT_RUNS):
        for n in ttft:
            ttft[n].append(once(n, f"{k}-{n}"))
    med = {n: statistics.median(v) for n, v in ttft.items()}
    for n, v in ttft.items():
        lines.append(f"time to first token, prompt_logprobs={n}: median {med[n]:8.1f} ms (min {min(v):8.1f} max {max(v):8.1f}, "
                     f"{TTFT_RUNS} runs, alternating)" + ("" if n is None else f"  added {med[n] - med[None]:7.1f} ms"))
    # the scoring rows in isolation, as ModelRunner._score slices them
    step = max(1, int(os.environ.get("LLMD_SCORE_ROWS", "256")))
    h = torch.randn(ISL - 1, cfg.model_config.hidden_size, device="cuda").to(torch.bfloat16)
    t32 = torch.randint(0, V, (ISL - 1,), device="cuda").int()
    logits = [eng.runner.model.compute_logits(h[a:a + step]) for a in range(0, ISL - 1, step)]
    for n in (0, 1):
        nn = torch.full((ISL - 1,), n, dtype=torch.int32, device="cuda")

        def gemm():
            for a in range(0, ISL - 1, step):
                eng.runner.model.compute_logits(h[a:a + step])

        def kern():
            for i, a in enumerate(range(0, ISL - 1, step)):
                ops.prompt_logprobs(logits[i], t32[a:a + step], nn[a:a + step])
        with torch.no_grad():
            for fn in (gemm, kern):
                fn()
            tg = statistics.median(window(gemm, 1) for _ in range(9)) / 1e3
            tk = statistics.median(window(kern, 1) for _ in range(9)) / 1e3
        lines.append(f"{ISL - 1} scoring rows in slices of {step}, n={n}: LM-head GEMM {tg:7.2f} ms, kernel {tk:7.2f} ms "
                     f"(device events, median of 9); the rest of the added time is the row gather, the copy of "
                     f"the results to the host and host work")
    eng.shutdown()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    lines = [f"# {torch.cuda.get_device_name(0)}"]
    kernel_table(lines)
    if "--kernel-only" not in sys.argv:
        end_to_end(lines)
    text = "\n".join(lines)
    print(text)
    if args:
        with open(args[0], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
