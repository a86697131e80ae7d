"""Times HiFi-GAN V3 (ResBlock2) on the fused residual-block launch -> profiles/vocoder_rb2_timing.json.

Workload: V3 with random weights, one 800-frame utterance and a batch of 8, precision bf16x3 (the default).  Every arm replays its
hipGraph (the stock-torch arms run eagerly: they have no capture path here); events around 10 calls, five rounds, all arms interleaved
in one process, after a warm-up of every arm.
  v3_fused       fused_resblock2 = True: one efts_resblock2 launch per residual block
  v3_composed    fused_resblock2 = False: blocks 0 and 1 of every stage as two efts_gemm launches, block 2 (k = 7, d = 12: beyond
                 efts_gemm) fused -- the closest composed arm there is
  v1             the shipped V1 generator in the same windows
  torch_fp32 / torch_bf16   the same V3 generator in stock torch ops (conv1d / conv_transpose1d), fp32 and under bf16 autocast
and efts_resblock2 alone per stage and block (events around 20 launches, five rounds): time, bytes over time against 8 TB/s.

DECISION RULE (written before the run): fused_resblock2 defaults to True only if the median of v3_fused is not above the median of
v3_composed by more than the spread (max - min) of the rounds; otherwise the default composes wherever composition can run.
"""
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from efficient_tts_amd import lib as L                      # noqa: E402
from efficient_tts_amd import ops as O                      # noqa: E402
from efficient_tts_amd.vocoder import HiFiGANGenerator      # noqa: E402

V3 = dict(resblock="2", upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8], upsample_initial_channel=256,
          resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]], num_mels=80)
V1 = dict(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
          resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80)
CALLS, ROUNDS, T = 10, 5, 800


def torch_v3(m: HiFiGANGenerator):
    """the V3 forward in stock torch ops on the module's own (folded) weights"""
    w = lambda c: (m._folded(c).float(), c.bias.detach().float())
    pre, post, ups = w(m.conv_pre), w(m.conv_post), [w(u) for u in m.ups]
    rbs = [[w(c) for c in rb.convs] for rb in m.resblocks]

    def run(mel):
        x = F.conv1d(mel, *pre, padding=3)
        n = 0
        for i, (u, k) in enumerate(zip(m.upsample_rates, m.upsample_kernel_sizes)):
            x = F.conv_transpose1d(F.leaky_relu(x, 0.1), *ups[i], stride=u, padding=(k - u) // 2)
            xs = None
            for j, kk in enumerate(m.res_kernels):
                r = x
                for t, d in enumerate(m.res_dilations[j]):
                    r = F.conv1d(F.leaky_relu(r, 0.1), *rbs[n][t], padding=(kk * d - d) // 2, dilation=d) + r
                xs = r if xs is None else xs + r
                n += 1
            x = xs / len(m.res_kernels)
        return torch.tanh(F.conv1d(F.leaky_relu(x), *post, padding=3))
    return run


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def launch_alone(dev, m_rows, c, k, d0, d1, sp=2):
    g = torch.Generator().manual_seed(c * 100 + k)
    x = torch.randn(m_rows, c, generator=g).to(dev)
    mask = torch.ones(m_rows, device=dev)
    p0 = O.Plane(64 + O.roundup(m_rows, 128) + 256, c, sp, dev, guard_lo=64)
    lib = L.load()
    with O.stream_scope():
        L.check(lib.efts_act_bwd(x.data_ptr(), x.data_ptr(), None, mask.data_ptr(), 0.1, 3, None, p0.ptr, p0.ld, sp, None, m_rows, c, O._stream()), "efts_act_bwd")
        pw = [O.PackedWeight(c, c, k, sp, dev) for _ in range(2)]
        for q in pw:
            q.pack((torch.randn(c, c, k, generator=g) / (c * k) ** 0.5).to(dev).contiguous())
    bias = torch.zeros(c, device=dev)
    out = torch.empty(m_rows, c, device=dev)
    a = L.ResBlock2Args()
    a.x, a.ldx, a.p0, a.ldp, a.w0, a.w1, a.ldw, a.w_tap_stride = x.data_ptr(), c, p0.ptr, p0.ld, pw[0].ptr, pw[1].ptr, pw[0].ld, pw[0].tap_stride
    a.bias0, a.bias1, a.rowmask, a.out, a.ldo = bias.data_ptr(), bias.data_ptr(), mask.data_ptr(), out.data_ptr(), c
    a.split, a.m, a.c, a.k, a.d0, a.d1, a.slope = sp, m_rows, c, k, d0, d1, 0.1
    st = torch.cuda.current_stream().cuda_stream
    fn = lambda: L.check(lib.efts_resblock2(ctypes.byref(a), st), "efts_resblock2")
    fn()
    torch.cuda.synchronize()
    ts = [timed(fn, 20) for _ in range(ROUNDS)]
    nbytes = m_rows * (c * 4 + p0.ld + c * 4 + 4)
    flops = 2 * 2 * m_rows * c * c * k
    med = statistics.median(ts)
    return dict(rows=m_rows, c=c, k=k, d=[d0, d1], us=[round(t * 1e3, 2) for t in ts], median_us=round(med * 1e3, 2),
                GBps=round(nbytes / med / 1e6, 1), hbm_fraction_of_8TBps=round(nbytes / med / 1e6 / 8000, 4), useful_TFLOPs=round(flops / med / 1e9, 2))


def main():
    L.require_device()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"workload": "HiFi-GAN V3, random weights, bf16x3, T = 800 frames; ms per call (events around 10 calls, 5 rounds, arms interleaved)",
           "decision_rule": "fused default only if median(v3_fused) <= median(v3_composed) + spread of the rounds"}
    for B in (1, 8):
        mel = torch.randn(B, 80, T, device=dev)
        fused = HiFiGANGenerator(V3).to(dev).eval()
        fused.fused_resblock2 = True
        comp = HiFiGANGenerator(V3).to(dev).eval()
        comp.load_state_dict(fused.state_dict())
        comp.fused_resblock2 = False
        v1 = HiFiGANGenerator(V1).to(dev).eval()
        tv3 = torch_v3(fused)

        def t32():
            with torch.no_grad():
                tv3(mel)

        def t16():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                tv3(mel)
        arms = {"v3_fused": lambda: fused(mel), "v3_composed": lambda: comp(mel), "v1": lambda: v1(mel), "torch_fp32": t32, "torch_bf16": t16}
        for fn in arms.values():                            # warm-up: packing, capture, autotuning of the stock ops
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        diff = float((fused(mel) - comp(mel)).abs().max())
        ts = {k: [] for k in arms}
        for _ in range(ROUNDS):
            for k, fn in arms.items():
                ts[k].append(timed(fn, CALLS))
        r = {k: dict(ms=[round(v, 4) for v in vs], median_ms=round(statistics.median(vs), 4), spread_ms=round(max(vs) - min(vs), 4)) for k, vs in ts.items()}
        r["max_abs_fused_minus_composed"] = diff
        res[f"B{B}"] = r
        print(B, {k: v["median_ms"] for k, v in r.items() if isinstance(v, dict)}, flush=True)
    f1, c1 = res["B1"]["v3_fused"], res["B1"]["v3_composed"]
    f8, c8 = res["B8"]["v3_fused"], res["B8"]["v3_composed"]
    ok = all(f["median_ms"] <= c["median_ms"] + max(f["spread_ms"], c["spread_ms"]) for f, c in ((f1, c1), (f8, c8)))
    res["decision"] = "fused_resblock2 defaults to True" if ok else "fused_resblock2 defaults to False (compose wherever composition can run)"
    rows, per = 800, []
    for i, (u, c) in enumerate(zip((8, 8, 4), (128, 64, 32))):
        rows *= u
        for j, (k, ds) in enumerate(zip(V3["resblock_kernel_sizes"], V3["resblock_dilation_sizes"])):
            e = launch_alone(dev, rows, c, k, ds[0], ds[1])
            e["stage"], e["block"] = i, j
            per.append(e)
            print(e, flush=True)
    res["efts_resblock2_alone_B1"] = per
    # (what, from the code, bounds the launch: DESIGN.md 4e; this file holds measured fields only)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "vocoder_rb2_timing.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(res["decision"])


if __name__ == "__main__":
    main()
