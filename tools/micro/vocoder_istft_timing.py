"""Times an iSTFTNet generator (C8C8I) against HiFi-GAN V1, and its head against stock torch -> profiles/vocoder_istft_timing.json.

Workload: random weights, one 800-frame utterance and a batch of 8, precision bf16x3 (the default).  The generator arms replay their
hipGraph; events around 10 calls, five rounds, all arms interleaved in one process, after a warm-up of every arm.
  c8c8i      upsample_rates [8, 8], gen_istft_n_fft 16, gen_istft_hop_size 4, 512 initial channels, V1's residual blocks: 256 samples per frame
  v1         the shipped V1 generator in the same windows
and the head alone on the z that the C8C8I arm left in its workspace (B x 51200 frames of 18 channels; events around 20 launches):
  efts_istft_head   the one launch (the reflected-row launch and conv_post are not in it)
  torch_head        torch.exp / sin / torch.istft on the same z on the same GPU, eagerly (the items at their pitch, z read in place)
Nothing is decided by this file: it reports (c8c8i against v1) and (the launch against torch_head) as measured.
"""
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from efficient_tts_amd import lib as L                      # noqa: E402
from efficient_tts_amd.vocoder import HiFiGANGenerator      # noqa: E402

V1 = dict(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
          resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80)
C8C8I = dict(V1, upsample_rates=[8, 8], upsample_kernel_sizes=[16, 16], gen_istft_n_fft=16, gen_istft_hop_size=4)
CALLS, ROUNDS, T = 10, 5, 800


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def stats(vs, unit="ms", scale=1.0):
    vs = [v * scale for v in vs]
    return {unit: [round(v, 4) for v in vs], f"median_{unit}": round(statistics.median(vs), 4), f"spread_{unit}": round(max(vs) - min(vs), 4)}


def head_arms(gen, B, dev):
    """the head launch and the stock-torch head on the z of the generator's last call"""
    N, h, rate = gen._head.n_fft, gen._head.hop, gen._rates[-1]
    ws = gen._workspace_for(B, T, dev)
    z, _ = ws.head
    pitch, frames = ws.pitch * rate, T * rate + 1
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    tab = gen._head.tables(dev)
    audio = torch.empty(B, 1, T * gen.hop, device=dev)
    a = L.IstftHeadArgs()
    a.mode, a.B, a.pitch, a.z, a.z_rows, a.lengths, a.len_mul = L.ISTFT_SYNTH, B, pitch, z.data_ptr(), B * pitch, lens.data_ptr(), rate
    a.window, a.twiddle, a.n_fft, a.hop = tab.data_ptr(), tab.data_ptr() + 4 * N, N, h
    a.audio, a.ld_audio, a.out_len = audio.data_ptr(), audio.shape[2], audio.shape[2]
    st = torch.cuda.current_stream().cuda_stream
    lib = L.load()
    window = torch.hann_window(N, device=dev)
    K = N // 2 + 1
    zv = z[:B * pitch].view(B, pitch, N + 2)[:, :frames]

    def torch_head():
        spec = torch.exp(zv[:, :, :K]) * torch.exp(1j * torch.sin(zv[:, :, K:]))
        return torch.istft(spec.transpose(1, 2), N, h, N, window=window, center=True)

    launch = lambda: L.check(lib.efts_istft_head(ctypes.byref(a), st), "efts_istft_head")
    launch()
    diff = float((torch_head() - audio[:, 0]).abs().max())
    return {"efts_istft_head": launch, "torch_head": torch_head}, diff, B * (frames * (N + 2) + T * gen.hop) * 4


def main():
    L.require_device()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"workload": "random weights, bf16x3, T = 800 frames; generators: ms per call (hipGraph replays, events around 10 calls, 5 rounds, arms "
                       "interleaved); head: us per call (events around 20 calls, eager)"}
    for B in (1, 8):
        mel = torch.randn(B, 80, T, device=dev)
        istft = HiFiGANGenerator(C8C8I).to(dev).eval()
        v1 = HiFiGANGenerator(V1).to(dev).eval()
        arms = {"c8c8i": lambda: istft(mel), "v1": lambda: v1(mel)}
        for fn in arms.values():                            # warm-up: packing, capture
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        heads, diff, nbytes = head_arms(istft, B, dev)
        for fn in heads.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in (*arms, *heads)}
        for _ in range(ROUNDS):
            for k, fn in arms.items():
                ts[k].append(timed(fn, CALLS))
            for k, fn in heads.items():
                ts[k].append(timed(fn, 2 * CALLS))
        r = {k: stats(ts[k]) for k in arms}
        r.update({k: stats(ts[k], "us", 1e3) for k in heads})
        r["c8c8i_over_v1"] = round(r["c8c8i"]["median_ms"] / r["v1"]["median_ms"], 4)
        r["efts_istft_head_over_torch_head"] = round(r["efts_istft_head"]["median_us"] / r["torch_head"]["median_us"], 4)
        r["head_bytes"] = nbytes
        r["head_GBps"] = round(nbytes / r["efts_istft_head"]["median_us"] / 1e3, 1)
        r["max_abs_launch_minus_torch_head"] = diff
        res[f"B{B}"] = r
        print(B, {k: v for k, v in r.items() if not isinstance(v, dict)}, {k: v.get("median_ms", v.get("median_us")) for k, v in r.items() if isinstance(v, dict)}, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "vocoder_istft_timing.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
