"""CPU: the reference of the vocoder stage tests (tests/vocoder_reference.py) is pinned, its cases are conditioned, and the
constructor refuses what the module cannot compute.

1. On the V1 configuration, with the oracle's parameters and the mels of tests/golden/hifigan_small.npz, the float64 `forward` equals
   oracle/hifigan_oracle.py:forward and the reference's golden audio within the 2e-5 of tests/test_vocoder.py, and composing the per-step
   functions by hand gives `forward` exactly.
2. For every case of tests/test_vocoder_stages_gpu.py, every step's float32 transcription meets FACTOR * e32 <= COND against float64
   (the condition `kernel_check._check` asserts next to a kernel's error), and no stage's max |ref| is below 1e-3 or above 1e3, so that
   a bound relative to max |ref| means something.
3. `HiFiGANGenerator.__init__` raises NotImplementedError, naming the reason, for every configuration `_run` would compute wrongly or
   fail on at its first launch.
"""
import os

import numpy as np
import pytest
import torch

import vocoder_reference as VR
from kernel_check import COND, FACTOR, conditioned
from oracle import hifigan_oracle as HO

GOLD = os.path.join(os.path.dirname(__file__), "golden", "hifigan_small.npz")


def test_reference_matches_oracle_and_golden_on_v1():
    g = np.load(GOLD)
    P = HO.fill_params()
    assert list(VR.param_shapes(VR.V1).items()) == list(HO.param_shapes().items())
    R = VR.Reference(VR.V1, P, torch.float64)
    for name in ("a", "b"):
        mel = torch.from_numpy(g[f"mel_{name}"])
        st = VR.forward(P, mel)
        y = st["out"]
        assert y.dtype == torch.float64 and y.shape == g[f"audio_{name}"].shape
        assert float((y - HO.forward(P, mel).double()).abs().max()) < 2e-5
        assert np.abs(y.numpy() - g[f"audio_{name}"]).max() < 2e-5
        # the per-step functions, composed by hand, are `forward`
        x = R.conv_pre(mel)
        assert torch.equal(x, st["pre"])
        for i in range(4):
            x = R.up(i, x)
            assert torch.equal(x, st[f"up{i}"])
            assert torch.equal(R.up(i, torch.nn.functional.leaky_relu(st["pre"] if i == 0 else st[f"mean{i - 1}"], 0.1), activated=True), x)
            finals = []
            for j in range(3):
                r = x
                for d_i in range(3):
                    r = R.res_pair(i * 3 + j, d_i, r)
                    assert torch.equal(r, st[f"r{i}.{j}.{d_i}"])
                finals.append(r)
            x = R.mean(finals)
            assert torch.equal(x, st[f"mean{i}"])
        assert torch.equal(R.conv_post(x), y)
        assert torch.equal(R.conv_post(torch.nn.functional.leaky_relu(x, 0.01), activated=True), y)


def test_reference_lengths_are_items_alone():
    cs = VR.CASES["narrow"]
    P = VR.fill(cs["cfg"], cs["seed"])
    mel = VR.mel_input(cs["cfg"], len(cs["lengths"]), cs["T"], cs["seed"])
    st = VR.forward(P, mel, cs["lengths"], cfg=cs["cfg"])
    for b, n in enumerate(cs["lengths"]):
        alone = VR.forward(P, mel[b:b + 1, :, :n], cfg=cs["cfg"])
        for name, v in alone.items():
            rate = v.shape[2] // n
            assert torch.equal(st[name][b, :, :n * rate], v[0]) and float(st[name][b, :, n * rate:].abs().max() if n < cs["T"] else 0.0) == 0.0


@pytest.mark.parametrize("case", list(VR.CASES))
def test_stage_cases_are_conditioned(case):
    cs = VR.CASES[case]
    P = VR.fill(cs["cfg"], cs["seed"])
    mel = VR.mel_input(cs["cfg"], len(cs["lengths"]), cs["T"], cs["seed"])
    refs = VR.step_refs(cs["cfg"], P, mel, cs["lengths"])
    full = VR.forward(P, mel, cs["lengths"], cfg=cs["cfg"])
    assert set(refs) == set(full)
    for name, (r64, r32) in refs.items():
        assert r64.dtype == torch.float64 and r32.dtype == torch.float32
        assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), f"{case} {name}"
        ok, e32 = conditioned(r64, r32)
        big = float(r64.abs().max())
        print(f"COND {case} {name} e32={e32:.3e} max|ref|={big:.3e}")
        assert ok, f"{case} {name}: e32 = {e32:.3e}, {FACTOR} * e32 > {COND}"
        assert 1e-3 <= big <= 1e3, f"{case} {name}: max |ref| = {big:.3e}"
    # the whole generator in float32 against float64: what `_check(chain=True)` measures the device's fp32 mode with
    e32 = conditioned(full["out"], VR.forward(P, mel, cs["lengths"], cfg=cs["cfg"], dtype=torch.float32)["out"])[1]
    print(f"COND {case} whole e32={e32:.3e}")
    assert e32 <= COND


# ------------------------------------------------------------------------------------------------------------------- refusals
_BASE = dict(resblock="1", upsample_rates=[4, 4], upsample_kernel_sizes=[8, 8], upsample_initial_channel=64,
             resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80)
REFUSED = {
    "four residual kernels": (dict(resblock_kernel_sizes=[3, 5, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 4), "efts_mean_act_rows"),
    "no residual kernel": (dict(resblock_kernel_sizes=[], resblock_dilation_sizes=[]), "efts_mean_act_rows"),
    "fewer dilation lists than kernels": (dict(resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5]]), "one list per entry"),
    "even residual kernel": (dict(resblock_kernel_sizes=[3, 4, 11]), "kernel size 4"),
    "residual kernel 13": (dict(resblock_kernel_sizes=[3, 7, 13]), "kernel size 13"),
    "halo past the window": (dict(resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 7]]), "(k - 1) * d <= 64"),
    "dilation 0": (dict(resblock_dilation_sizes=[[1, 3, 5], [0, 3, 5], [1, 3, 5]]), "d >= 1"),
    "empty dilation list": (dict(resblock_dilation_sizes=[[1, 3, 5], [], [1, 3, 5]]), "empty dilation list"),
    "kernel != 2 * stride": (dict(upsample_kernel_sizes=[8, 6]), "kernel = 2 * stride"),
    "odd stride": (dict(upsample_rates=[4, 3], upsample_kernel_sizes=[8, 6]), "even stride"),
    "rates and kernels differ in length": (dict(upsample_kernel_sizes=[8]), "one length"),
    "no upsampling stage": (dict(upsample_rates=[], upsample_kernel_sizes=[]), "non-empty"),
    "channels not a multiple of 4": (dict(upsample_initial_channel=24), "multiple of 4"),
    "channels do not halve": (dict(upsample_initial_channel=50), "multiple of 4"),
    "ResBlock2": (dict(resblock="2"), "ResBlock1"),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_constructor_refuses_what_it_cannot_compute(what):
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    change, reason = REFUSED[what]
    with pytest.raises(NotImplementedError) as e:
        HiFiGANGenerator(dict(_BASE, **change))
    assert reason in str(e.value), (what, str(e.value))


def test_constructor_accepts_the_stage_cases_and_derives_the_gap():
    """the gap between the items of a batch follows from the configuration: its rows at the first upsampled stage hold the largest
    residual halo, (11 - 1) / 2 * 5 = 25 rows where a k = 11, d = 5 convolution exists; V1 stays at 4 frames"""
    from efficient_tts_amd.vocoder import HiFiGANGenerator, gap_frames
    want = {"narrow": 4, "v2ish": 13, "gap": 7, "resident": 7, "v1-small": 4}
    for name, cs in VR.CASES.items():
        m = HiFiGANGenerator(cs["cfg"])
        assert m.gap_frames == want[name], name
        halo = max((k - 1) // 2 * d for k, ds in zip(m.res_kernels, m.res_dilations) for d in ds)
        assert m.gap_frames * m.upsample_rates[0] >= halo and m.gap_frames >= 4
        assert list(m.state_dict().keys()) == list(VR.param_shapes(cs["cfg"]).keys())
        assert all(tuple(v.shape) == VR.param_shapes(cs["cfg"])[k] for k, v in m.state_dict().items())
    assert gap_frames((8, 8, 2, 2), (3, 7, 11), ((1, 3, 5),) * 3) == 4
    assert gap_frames((2, 2), (11,), ((1, 5),)) == 13 and gap_frames((4, 4), (3, 7, 11), ((1, 3, 5),) * 3) == 7
