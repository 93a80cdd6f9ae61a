"""A/B timing of HexConvTranspose2d at radius 2, stride 2: the matrix-core kernel k_hexconvt_s2
(csrc/conv_transpose_mfma.hip) against the layer's adjoint route (the generic d-input gather of
csrc/hexconv_bwd.hip plus a bias add, selected by HYGRID_CONVT_MFMA=0), interleaved in one
process, HIP events on the launch stream, median over rounds with the spread (min .. max) of
each side.  Shapes: the adjoints of the stride-2 forward table of DESIGN.md 8 (in -> out, output
size, batch), with bf16 x -> bf16 y and f32 x -> f32 y; the 16 -> 16 shape decides the
out_channels threshold; 64 -> 3 stays on the adjoint route and is recorded alone.  Next to each:
the f32 stride-2 forward of the adjoint HexConv2d (out -> in channels on the output image), which
has the same FLOPs (2 * 7 * in * out * B * hin * win).  One JSON line per case.

usage: python tools/ab_conv_transpose.py [rounds]      (default 6)
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hybrid-grid-for-hexagonal-and-rectangular-image-processing_amd")]

import torch  # noqa: E402

from HyGrid import _abi, ops  # noqa: E402

SWITCH = "HYGRID_CONVT_MFMA"
PEAK_F32_MFMA = 157.3
SHAPES = [(4, 128, 64, 1080, 1920), (2, 256, 128, 540, 960), (8, 16, 16, 540, 960),
          (4, 64, 3, 1080, 1920)]                       # (B, in, out, h, w), padding 1


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def side(t, flop):
    ms = statistics.median(t)
    return {"ms": round(ms, 4), "min": round(min(t), 4), "max": round(max(t), 4),
            "spread": round(max(t) - min(t), 4), "TFLOPs": round(flop / ms / 1e9, 2)}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(2)
    for B, ci, co, h, w in SHAPES:
        hin, win = ops.hexconv2d_out_shape(h, w, 2, 2, 1, 1)
        k = (torch.rand((ci, co, 1, 7), generator=g, device=dev) - 0.5) / (2 * ci) ** 0.5
        b = torch.rand((co,), generator=g, device=dev) - 0.5
        flop = 2.0 * 7 * ci * co * B * hin * win
        base = {"batch": B, "in": ci, "out": co, "hin": hin, "win": win, "h": h, "w": w}
        # the adjoint conv's f32 stride-2 forward on the same machine
        u = torch.rand((B, co, h, w), generator=g, device=dev) - 0.5
        t = [timed(lambda: ops.hexconv2d(u, k, None, 0, 2, 2, 1, out_dtype=torch.float32))
             for _ in range(rounds + 1)][1:]
        fwd = side(t, flop)
        fwd["plan"] = ops.hexconv2d_forward_plan(u.dtype, k.dtype, torch.float32, B, co, ci, h, w,
                                                 2, 2, 1)
        print(json.dumps(dict(base, run="forward_f32_of_adjoint_conv", **fwd)), flush=True)
        del u
        for xd in (torch.bfloat16, torch.float32):
            x = (torch.rand((B, ci, hin, win), generator=g, device=dev) - 0.5).to(xd)
            plan = ops.hexconv_transpose2d_plan(xd, k.dtype, xd, B, ci, co, hin, win, h, w, 2, 2, 1)
            modes = ("1", "0") if plan == _abi.HG_CONVT_MFMA_S2 else ("0",)
            res = {}
            for r in range(rounds + 1):
                for mode in modes:
                    os.environ[SWITCH] = mode
                    ms = timed(lambda: ops.hexconv_transpose2d(x, k, b, 0, 2, 2, 1, 1, 1, (h, w), xd))
                    if r:
                        res.setdefault(mode, []).append(ms)
            os.environ.pop(SWITCH, None)
            out = dict(base, run="transpose", x=str(xd), y=str(xd), plan=plan)
            out["adjoint"] = side(res["0"], flop)
            if "1" in res:
                out["mfma"] = side(res["1"], flop)
                out["mfma"]["frac_f32_mfma_peak"] = round(out["mfma"]["TFLOPs"] / PEAK_F32_MFMA, 3)
                gain = out["adjoint"]["ms"] - out["mfma"]["ms"]
                out["speedup"] = round(out["adjoint"]["ms"] / out["mfma"]["ms"], 2)
                out["faster_by_more_than_spread"] = bool(
                    gain > max(out["adjoint"]["spread"], out["mfma"]["spread"]))
                out["ms_over_forward"] = round(out["mfma"]["ms"] / fwd["ms"], 2)
            print(json.dumps(out), flush=True)
            del x


if __name__ == "__main__":
    main()
