"""Wide-channel HexConv2d (HexConvModule in segmentation models, HexModules.py:97-288):
the MFMA implicit-GEMM kernels (conv_mfma.hip) against the generic LDS kernel
(HYGRID_CONV_MFMA=0), one process, the two sides interleaved round by round, HIP events, median
over rounds; TFLOP/s counted as 2*O*7*C per output sample (the dense hex contraction; the output
sample count from hexconv2d_out_shape), against the f32 matrix peak (157.3 TF), for bf16 inputs
also against the bf16 matrix peak (2500 TF: the split-weight kernel issues up to three bf16
MFMAs per counted product).

spread: the timed rounds of a side are dealt into three groups; the spread is the largest minus the
smallest group median.  `wins`: the MFMA median is below the generic median by more than the sum of
the two spreads.

usage: python tools/bench_conv_wide.py [rounds [stride]]     -> one JSON line per shape
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hybrid-grid-for-hexagonal-and-rectangular-image-processing_amd")]

import torch  # noqa: E402

from HyGrid import ops  # noqa: E402

F32_MFMA_PEAK_TF = 157.3
BF16_MFMA_PEAK_TF = 2500.0
GENERIC_ROUNDS = 6          # the generic kernel is slow: two timed rounds per spread group

SHAPES = {  # stride -> (B, C, O, H, W)
    1: [(4, 64, 64, 1080, 1920), (8, 32, 32, 540, 960), (2, 128, 128, 540, 960),
        (4, 16, 32, 1080, 1920)],
    # a downsampling conv, the 3-channel stem, the routing threshold, a deep stage
    2: [(4, 64, 128, 1080, 1920), (4, 3, 64, 1080, 1920), (8, 16, 16, 540, 960),
        (2, 128, 256, 540, 960)],
}
KERNEL_NAMES = ["other", "mfma_f32", "mfma_bf16", "mfma_bf16_dma"]


def _spread(ts):
    groups = [ts[i::3] for i in range(3) if ts[i::3]]
    meds = [statistics.median(g) for g in groups]
    return max(meds) - min(meds)


def run(B, C, O, H, W, dt, rounds, stride):
    dev = torch.device("cuda:0")
    x = (torch.rand((B, C, H, W), device=dev) - 0.5).to(dt)
    k = (torch.rand((O, C, 1, 7), device=dev) - 0.5) * 0.1
    b = torch.rand((O,), device=dev) - 0.5
    res = {}
    for r in range(rounds + 1):
        for mode in ("1", "0"):
            if mode == "0" and r > GENERIC_ROUNDS:
                continue
            os.environ["HYGRID_CONV_MFMA"] = mode
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.hexconv2d(x, k, b, 0, 2, stride=stride, padding=1, out_dtype=dt)
            e1.record()
            e1.synchronize()
            if r:
                res.setdefault(mode, []).append(e0.elapsed_time(e1))
    os.environ.pop("HYGRID_CONV_MFMA", None)
    ho, wo = ops.hexconv2d_out_shape(H, W, 2, stride, 1, 1)
    flops = 2.0 * O * 7 * C * B * ho * wo
    kern = ops.hexconv2d_forward_plan(dt, torch.float32, dt, B, C, O, H, W, 2, stride=stride, padding=1)
    out = {"shape": f"B{B} C{C} O{O} {H}x{W}", "stride": stride, "dtype": str(dt),
           "kernel": KERNEL_NAMES[kern]}
    for mode, name in (("1", "mfma"), ("0", "generic")):
        ms = statistics.median(res[mode])
        out[name] = {"ms": round(ms, 4), "spread_ms": round(_spread(res[mode]), 4),
                     "rounds": len(res[mode]), "TFLOP_s": round(flops / ms / 1e9, 2)}
    out["mfma"]["frac_f32_mfma_peak"] = round(out["mfma"]["TFLOP_s"] / F32_MFMA_PEAK_TF, 4)
    if dt == torch.bfloat16:
        out["mfma"]["frac_bf16_mfma_peak"] = round(out["mfma"]["TFLOP_s"] / BF16_MFMA_PEAK_TF, 4)
    out["speedup"] = round(out["generic"]["ms"] / out["mfma"]["ms"], 2)
    out["wins"] = bool(out["mfma"]["ms"] + out["mfma"]["spread_ms"] + out["generic"]["spread_ms"]
                       < out["generic"]["ms"])
    print(json.dumps(out), flush=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    stride = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    for (B, C, O, H, W) in SHAPES[stride]:
        for dt in (torch.bfloat16, torch.float32):
            run(B, C, O, H, W, dt, rounds, stride)


if __name__ == "__main__":
    main()
