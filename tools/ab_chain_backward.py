"""A/B of one training step of the chain rect -> hex -> HexConv2d -> hex -> rect: the fused
forward + fused backward (rect_hex_conv_rect(fused=True), hg_pipeline_r2h_conv_h2r and
hg_pipeline_r2h_conv_h2r_backward) against the operator chain and its three generic backward
kernels (fused=False).  A step is forward + backward() with conv.kernel and conv.bias
requiring grad and x not (--x-grad: x too, which adds the input pass).

Both variants run in ONE process, alternating: each repetition times `steps` steps of one
variant between two HIP events (the second followed by a synchronise), then the same for the
other.  Peak memory (torch.cuda.max_memory_allocated over a step, inputs included) is measured
per variant after a reset of the peak counter.

usage: python tools/ab_chain_backward.py [--batch 16] [--reps 3] [--steps 20] [--warmup 3]
                                         [--height 2160] [--width 3840] [--x-grad] [--out FILE]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hybrid-grid-for-hexagonal-and-rectangular-image-processing_amd"))

from HyGrid.HexFrames import HexConv2d  # noqa: E402
from HyGrid.pipeline import rect_hex_conv_rect  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--x-grad", action="store_true", help="x requires grad too (adds the input pass)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    conv = HexConv2d(3, 3, 0, 2, padding=1, bias=True).to(dev).train()
    gen = torch.Generator(device=dev).manual_seed(2)
    shape = (a.batch, 3, a.height, a.width)
    x = torch.rand(shape, generator=gen, device=dev, dtype=torch.bfloat16)
    g = torch.rand(shape, generator=gen, device=dev, dtype=torch.bfloat16)
    x.requires_grad_(a.x_grad)

    def step(fused):
        conv.zero_grad(set_to_none=True)
        x.grad = None
        y = rect_hex_conv_rect(x, conv, fused=fused)
        y.backward(g)

    def timed(fused):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            step(fused)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.steps

    variants = (("fused", True), ("operators", False))
    peak, grads = {}, {}
    for name, fused in variants:
        for _ in range(a.warmup):
            step(fused)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step(fused)
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated()
        grads[name] = (conv.kernel.grad.clone(), conv.bias.grad.clone())
    times = {name: [] for name, _ in variants}
    for _ in range(a.reps):
        for name, fused in variants:
            times[name].append(timed(fused))
    torch.cuda.synchronize()

    rel = max(float((grads["fused"][i] - grads["operators"][i]).abs().max()
                    / grads["operators"][i].abs().max()) for i in (0, 1))
    what = "d kernel + d bias + d x" if a.x_grad else "d kernel + d bias"
    lines = [f"training step (forward + backward, {what}), {torch.cuda.get_device_name(0)}, "
             f"x {tuple(shape)} bf16, {a.reps} alternating repetitions of {a.steps} steps, "
             f"{a.warmup} warm-up steps"]
    for name, _ in variants:
        ts = times[name]
        lines.append(f"{name:10s} ms/step: " + " ".join(f"{t:.3f}" for t in ts)
                     + f"   min {min(ts):.3f} max {max(ts):.3f}   peak memory "
                     + f"{peak[name] / 2 ** 30:.2f} GiB")
    lines.append(f"slowest fused / fastest operators = "
                 f"{max(times['fused']) / min(times['operators']):.3f}; peak memory fused / "
                 f"operators = {peak['fused'] / peak['operators']:.3f}; "
                 f"max rel. difference of the gradients {rel:.2e}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
