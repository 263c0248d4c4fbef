"""Cost of ops.top_logprobs (csrc/ops/logprobs.hip) at serving shapes: V = 128256 bf16 logits,
B = 64 and 256, n = 5 and 20, against ops.sample on the same tensor and against the PyTorch
composition the engine would call without the kernel, log_softmax(x.float()).topk(20).
Each figure is the median over WINDOWS device-event windows of PER launches each, after a
warm-up; the three candidates alternate window by window, and the whole table is taken
REPEATS times so the run-to-run spread shows.
  python scripts/bench_top_logprobs.py [out.txt]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmd_amd import ops  # noqa: E402

V, WINDOWS, PER, REPEATS = 128256, 25, 10, 3


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(PER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / PER  # us per launch


def main():
    lines = [f"# {torch.cuda.get_device_name(0)}; V={V} bf16 randn*3; us per call, median of {WINDOWS} windows "
             f"x {PER} launches, candidates alternating; {REPEATS} repeats of every row"]
    x_all = (torch.randn(256, V, generator=torch.Generator().manual_seed(0)) * 3).to(torch.bfloat16).cuda()
    for B in (64, 256):
        x = x_all[:B]
        for n in (5, 20):
            nn = torch.full((B,), n, dtype=torch.int32, device="cuda")
            fns = {"top_logprobs": lambda: ops.top_logprobs(x, nn),
                   "sample": lambda: ops.sample(x, want_logprob=True),
                   "torch_topk20": lambda: torch.log_softmax(x.float(), -1).topk(20)}
            ids, lp = ops.top_logprobs(x, nn)
            rv, ri = torch.log_softmax(x.float(), -1).topk(20)
            assert (lp[:, :n] - rv[:, :n]).abs().max().item() < 1e-3  # values agree (tie order may differ in torch)
            for rep in range(REPEATS):
                for fn in fns.values():
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                t = {k: [] for k in fns}
                for _ in range(WINDOWS):
                    for k, fn in fns.items():
                        t[k].append(window(fn))
                med = {k: statistics.median(v) for k, v in t.items()}
                lines.append(f"B={B:3d} n={n:2d} rep{rep}: " + "  ".join(
                    f"{k} {med[k]:7.1f} (min {min(t[k]):6.1f} max {max(t[k]):6.1f})" for k in fns)
                    + f"  torch/kernel {med['torch_topk20'] / med['top_logprobs']:.2f}x")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
