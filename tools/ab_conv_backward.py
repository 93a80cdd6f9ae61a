"""A/B timing of the HexConv2d backward of wide layers: the matrix-core kernels
(csrc/conv_mfma_bwd.hip) against the generic kernels (csrc/hexconv_bwd.hip, selected by
HYGRID_CONV_BWD_MFMA=0), interleaved in one process, HIP events on the launch stream, median
over rounds.  Shapes: the bench's two wide layers, HexConv2d(64, 64, 0, 2, padding=1) and
HexConv2d(3, 64, 0, 2, padding=1) on 4 x C x 1080 x 1920 bf16 x with f32 gy, and two layers at
the routing thresholds, (16, 16) and (3, 16), on 4 x C x 270 x 480.  Runs: d input only,
d kernel + d bias only, all three; plus the forward (bf16 and f32 x) for scale.  One JSON line
per case: ms and algorithmic TFLOP/s (2 * O * 7 * C * B * h * w per gradient), for the MFMA
side also as a fraction of the 157.3 TFLOP/s f32-MFMA peak.

--stride 2: the stride-2 training routes of ops.hexconv2d_grads against the generic kernels
(what hg_hexconv2d_backward runs for a strided layer), interleaved in the same way by flipping
HYGRID_CONV_BWD_MFMA_S2 (d kernel / d bias: k_hexconv_bwd_weight_mfma_s2) and HYGRID_CONVT_MFMA
(d input: k_hexconvt_s2 on gy).  Shapes: the stride-2 forward table's, 64 -> 128 at 1080p b4,
128 -> 256 at 540p b2, 16 -> 16 at 540p b8 (the threshold) and the 3 -> 64 stem at 1080p b4
(d kernel only), bf16 x, f32 gy, padding 1.  Per gradient one JSON line: median, min and max ms
of each side, and whether the routed side wins by more than the two spreads combined.

usage: python tools/ab_conv_backward.py [rounds] [--stride 2]   (default 3 rounds: the generic
side is slow)
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hybrid-grid-for-hexagonal-and-rectangular-image-processing_amd")]

import torch  # noqa: E402

from HyGrid import ops  # noqa: E402

SWITCH = "HYGRID_CONV_BWD_MFMA"
PEAK_F32_MFMA = 157.3
SHAPES = [(4, 64, 64, 1080, 1920), (4, 3, 64, 1080, 1920), (4, 16, 16, 270, 480), (4, 3, 16, 270, 480)]
RUNS = [("dx", (True, False, False)), ("dk_db", (False, True, True)), ("all", (True, True, True))]
CFG = dict(off=0, r=2, stride=1, pad=1, dilation=1, groups=1, padding_mode="constant",
           padding_value=0.0, out_dtype=None)


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


S2_SWITCHES = {"dx": "HYGRID_CONVT_MFMA", "dk_db": "HYGRID_CONV_BWD_MFMA_S2"}
S2_SHAPES = [(4, 64, 128, 1080, 1920), (2, 128, 256, 540, 960), (8, 16, 16, 540, 960),
             (4, 3, 64, 1080, 1920)]
S2_CFG = dict(CFG, stride=2)


def main_stride2(rounds):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(2)
    for B, C, O, h, w in S2_SHAPES:
        x = (torch.rand((B, C, h, w), generator=g, device=dev) - 0.5).bfloat16()
        k = (torch.rand((O, C, 1, 7), generator=g, device=dev) - 0.5) / (7 * C) ** 0.5
        b = torch.rand((O,), generator=g, device=dev) - 0.5
        ho, wo = ops.hexconv2d_out_shape(h, w, 2, 2, 1, 1)
        gy = torch.randn((B, O, ho, wo), generator=g, device=dev)
        flop = 2.0 * O * 7 * C * B * ho * wo
        plan = ops.hexconv2d_training_plan(x.dtype, k.dtype, B, C, O, h, w, 2, 2, 1)
        for name, need in RUNS[:2]:
            if name == "dx" and plan[0] != "convt_s2":
                continue
            switch = S2_SWITCHES[name]
            res = {}
            for r in range(rounds + 1):
                for mode in ("1", "0"):
                    os.environ[switch] = mode
                    ms = timed(lambda: ops.hexconv2d_grads(gy, x, k, b, S2_CFG, *need))
                    if r:
                        res.setdefault(mode, []).append(ms)
            os.environ.pop(switch, None)
            out = dict(batch=B, C=C, O=O, h=h, w=w, stride=2, run=name, x="torch.bfloat16",
                       gy="torch.float32", plan={"dx": plan[0], "dk": plan[1]})
            for mode, t in res.items():
                ms = statistics.median(t)
                side = {"ms": round(ms, 4), "min": round(min(t), 4), "max": round(max(t), 4),
                        "TFLOPs": round(flop / ms / 1e9, 2)}
                if mode == "1":
                    side["frac_f32_mfma_peak"] = round(flop / ms / 1e9 / PEAK_F32_MFMA, 3)
                out["mfma" if mode == "1" else "generic"] = side
            spread = sum(max(t) - min(t) for t in res.values())
            gain = statistics.median(res["0"]) - statistics.median(res["1"])
            out["speedup"] = round(statistics.median(res["0"]) / statistics.median(res["1"]), 2)
            out["beats_spreads"] = bool(gain > spread)
            print(json.dumps(out), flush=True)
        del x, gy


def main():
    args = [a for a in sys.argv[1:]]
    stride = 1
    if "--stride" in args:
        i = args.index("--stride")
        stride = int(args[i + 1])
        del args[i:i + 2]
    rounds = int(args[0]) if args else 3
    if stride == 2:
        return main_stride2(rounds)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(2)
    for B, C, O, h, w in SHAPES:
        x = (torch.rand((B, C, h, w), generator=g, device=dev) - 0.5).bfloat16()
        k = (torch.rand((O, C, 1, 7), generator=g, device=dev) - 0.5) / (7 * C) ** 0.5
        b = torch.rand((O,), generator=g, device=dev) - 0.5
        ho, wo = ops.hexconv2d_out_shape(h, w, 2, 1, 1, 1)
        gy = torch.randn((B, O, ho, wo), generator=g, device=dev)
        flop = 2.0 * O * 7 * C * B * h * w
        base = {"batch": B, "C": C, "O": O, "h": h, "w": w}
        plan = ops.hexconv2d_backward_plan(x.dtype, k.dtype, B, C, O, h, w, 2, padding=1)
        # the forward, for scale: bf16 x on the bf16 split-weight kernel, f32 x on the f32 one
        for xd in (torch.bfloat16, torch.float32):
            xf = x.to(xd)
            t = [timed(lambda: ops.hexconv2d(xf, k, b, 0, 2, padding=1, out_dtype=xd))
                 for _ in range(rounds + 1)][1:]
            ms = statistics.median(t)
            print(json.dumps(dict(base, run="forward", x=str(xd), ms=round(ms, 4),
                                  TFLOPs=round(flop / ms / 1e9, 2),
                                  frac_f32_mfma_peak=round(flop / ms / 1e9 / PEAK_F32_MFMA, 3))),
                  flush=True)
            del xf
        for name, need in RUNS:
            ngrad = int(need[0]) + int(need[1])
            res = {}
            for r in range(rounds + 1):
                for mode in ("1", "0"):
                    os.environ[SWITCH] = mode
                    ms = timed(lambda: ops.hexconv2d_backward(gy, x, k, b, CFG, *need))
                    if r:
                        res.setdefault(mode, []).append(ms)
            os.environ.pop(SWITCH, None)
            out = dict(base, run=name, x="torch.bfloat16", gy="torch.float32",
                       plan={"dx": plan[0], "dk": plan[1]})
            for mode, t in res.items():
                ms = statistics.median(t)
                tf = ngrad * flop / ms / 1e9
                side = {"ms": round(ms, 4), "TFLOPs": round(tf, 2)}
                if mode == "1":
                    side["frac_f32_mfma_peak"] = round(tf / PEAK_F32_MFMA, 3)
                out["mfma" if mode == "1" else "generic"] = side
            out["speedup"] = round(statistics.median(res["0"]) / statistics.median(res["1"]), 2)
            print(json.dumps(out), flush=True)
        del x, gy


if __name__ == "__main__":
    main()
