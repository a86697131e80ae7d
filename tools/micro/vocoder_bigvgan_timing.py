"""Times `efts_snake_aa`, BigVGAN's anti-aliased Snake activation as one launch -> profiles/bigvgan_timing.json.

The launch alone at the four stage shapes of BigVGAN's base configuration (800 frames: rows x c = 6 400 x 256, 51 200 x 128, 102 400 x 64,
204 800 x 32), one utterance and eight, fp32 rows in and a bf16x3 plane out, against the torch-op composition of the same activation
(grouped conv_transpose1d, sin, grouped strided conv1d, two pads, a crop) on the same GPU in fp32 and under bf16 autocast.  All arms eager,
events around 20 launches, five rounds, arms interleaved, median with min .. max.  Reported: the largest difference between the launch's
fp32 output and the fp32 composition, bytes (fp32 in, plane out) over time as a share of 8 TB/s.
`--label` names the build of the library (for example the `sin` variant, -DEFTS_SNAKE_FAST_SIN) in the file; `--out` another file name.
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from efficient_tts_amd import lib as L                      # noqa: E402
from efficient_tts_amd import ops as O                      # noqa: E402

ROUNDS = 5
SHAPES = ((6400, 256), (51200, 128), (102400, 64), (204800, 32))


def aa_filter() -> torch.Tensor:
    """float64 [12]: the Kaiser-windowed sinc of include/efts_abi.h (cutoff 0.25, half-width 0.3), sum 1"""
    beta = 0.1102 * (2.285 * 5 * math.pi * 1.2 + 7.95 - 8.7)
    w = torch.kaiser_window(12, periodic=False, beta=beta, dtype=torch.float64)
    f = 0.5 * w * torch.sinc(0.5 * (torch.arange(12, dtype=torch.float64) - 5.5))
    return f / f.sum()


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def stats(vs, scale=1.0, nd=4):
    return dict(median=round(statistics.median(vs) * scale, nd), min=round(min(vs) * scale, nd), max=round(max(vs) * scale, nd))


def activation_torch(x, a, inv_b, f):
    """Activation1d on [B, C, L] in stock torch ops"""
    C = x.shape[1]
    u = 2 * F.conv_transpose1d(F.pad(x, (5, 5), mode="replicate"), f.expand(C, -1, -1), stride=2, groups=C)[..., 15:-15]
    v = u + inv_b.view(1, C, 1) * torch.sin(u * a.view(1, C, 1)) ** 2
    return F.conv1d(F.pad(v, (5, 6), mode="replicate"), f.expand(C, -1, -1), stride=2, groups=C)


def launch_alone(dev, B, rows, c, sp=2):
    g = torch.Generator().manual_seed(rows + c)
    x = (2 * torch.randn(B * rows, c, generator=g)).to(dev)
    a, inv_b = torch.exp(0.5 * torch.randn(c, generator=g)).to(dev), torch.exp(0.5 * torch.randn(c, generator=g)).to(dev)
    lens = torch.full((B,), rows, dtype=torch.int32, device=dev)
    plane = O.Plane(B * rows, c, sp, dev)
    out = torch.empty(B * rows, c, device=dev)
    f = aa_filter().float().view(1, 1, 12).to(dev)
    k = L.SnakeAAArgs()
    k.x, k.ldx, k.lengths, k.a, k.inv_b = x.data_ptr(), c, lens.data_ptr(), a.data_ptr(), inv_b.data_ptr()
    k.plane, k.ld_plane, k.split = plane.ptr, plane.ld, sp
    k.B, k.pitch, k.T, k.len_mul, k.c = B, rows, rows, 1, c
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    x_bcl = x.view(B, rows, c).transpose(1, 2).contiguous()

    def t32():
        with torch.no_grad():
            return activation_torch(x_bcl, a, inv_b, f)

    def t16():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return activation_torch(x_bcl, a, inv_b, f)
    arms = {"efts_snake_aa": lambda: L.check(lib.efts_snake_aa(ctypes.byref(k), st), "efts_snake_aa"), "torch_fp32": t32, "torch_bf16": t16}
    # agreement: the launch's fp32 output against the fp32 composition
    k2 = L.SnakeAAArgs.from_buffer_copy(k)
    k2.plane, k2.out, k2.ldo = None, out.data_ptr(), c
    L.check(lib.efts_snake_aa(ctypes.byref(k2), st), "efts_snake_aa")
    ref = t32().transpose(1, 2).reshape(B * rows, c)
    agree = float((out - ref).abs().max()) / float(ref.abs().max())
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n in arms}
    for _ in range(ROUNDS):
        for n, fn in arms.items():
            ts[n].append(timed(fn, 20))
    nbytes = B * rows * (c * 4 + plane.ld)
    med = statistics.median(ts["efts_snake_aa"])
    return dict(B=B, rows=rows, c=c, us={n: stats(v, 1e3, 2) for n, v in ts.items()}, max_rel_diff_vs_torch_fp32=agree,
                bytes=nbytes, GBps=round(nbytes / med / 1e6, 1), hbm_fraction_of_8TBps=round(nbytes / med / 1e6 / 8000, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="sinf (the shipped build)")
    ap.add_argument("--out", default="bigvgan_timing.json")
    args = ap.parse_args()
    L.require_device()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"library": args.label, "segment_rows": L.SNAKE_SEG,
           "method": "events around 20 launches, 5 rounds, arms interleaved in one process; median, min, max",
           "counters": "none read"}
    res["launch_alone"] = []
    for B in (1, 8):
        for rows, c in SHAPES:
            e = launch_alone(dev, B, rows, c)
            res["launch_alone"].append(e)
            print(e, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", args.out), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
