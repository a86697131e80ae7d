"""GPU (-m gpu): `efts_denoise` through `BiasDenoiser` against the float64 definition of tests/denoise_reference.py on one ragged batch; the
error bound is not fixed by hand but computed: four times what the same pipeline through torch.stft / torch.istft in fp32 on the CPU loses
against that reference on the same inputs.  Then the structure of the output, invariance, behaviour on a hum, `from_vocoder` and capture.
"""
import json
import os

import numpy as np
import pytest
import torch

import denoise_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _denoiser(strength=0.5):
    from efficient_tts_amd.denoise import BiasDenoiser
    return BiasDenoiser(DEV, R.bias_spectrum(), strength=strength)


def _batch():
    audio, lengths = R.batch()
    return torch.from_numpy(audio).to(DEV), torch.from_numpy(lengths).to(DEV)


def test_parity_with_the_float64_reference_within_four_times_the_fp32_yardstick():
    ref, share = R.reference_batch()
    assert 0.05 <= share <= 0.95                                       # both branches of the gain are exercised (checked on the reference)
    yard = R.yardstick()
    audio, lengths = _batch()
    d = _denoiser()
    worst = 0.0
    for s in R.STRENGTHS:
        out = d(audio, lengths, strength=s).cpu().numpy().astype(np.float64)
        for b, n in enumerate(R.LENGTHS):
            if n:
                worst = max(worst, float(np.abs(out[b, :n] - ref[s][b]).max()))
    print(f"max |device - reference| = {worst:.3e}; fp32 torch.stft / istft on the CPU: {yard:.3e}; bound 4 x = {4 * yard:.3e}")
    if os.environ.get("EFTS_WRITE_PROFILES"):                          # how profiles/denoise_error.json is produced
        with open(os.path.join(ROOT, "profiles", "denoise_error.json"), "w") as f:
            json.dump({"device_max_abs_error": worst, "yardstick_fp32_torch_cpu_max_abs_error": yard, "bound": 4 * yard,
                       "lengths": list(R.LENGTHS), "strengths": list(R.STRENGTHS), "clamped_share_at_0.5": share}, f)
            f.write("\n")
    assert 0.0 < yard < 1e-6                                           # the yardstick itself is an fp32 rounding error on signals of peak 0.5
    assert worst <= 4 * yard


def test_structure_of_the_output():
    audio, lengths = _batch()
    out, frames = _denoiser()(audio, lengths, return_frames=True)
    assert out.shape == audio.shape and out.dtype == torch.float32 and frames.dtype == torch.int32
    assert frames.tolist() == [1 + n // 256 if n > 512 else 0 for n in R.LENGTHS]
    for b, n in enumerate(R.LENGTHS):
        assert float(out[b, n:].abs().max()) == 0.0
        if n <= 512:
            assert torch.equal(out[b, :n], audio[b, :n])
        else:
            assert not torch.equal(out[b, :n], audio[b, :n])


def test_every_item_alone_twice_and_with_nan_behind_it_gives_the_same_bits():
    audio, lengths = _batch()
    d = _denoiser()
    out = d(audio, lengths)
    assert torch.equal(d(audio, lengths), out)
    for b, n in enumerate(R.LENGTHS):
        alone = d(audio[b:b + 1], lengths[b:b + 1])
        assert torch.equal(alone[0], out[b]), b
        if n > 512:                                                    # and in a buffer of its own size, with no lengths given
            assert torch.equal(d(audio[b:b + 1, :n].contiguous())[0], out[b, :n]), b
    poisoned = audio.clone()
    for b, n in enumerate(R.LENGTHS):
        poisoned[b, n:] = float("nan")
    assert torch.equal(d(poisoned, lengths), out)
    perm = torch.tensor([6, 0, 5, 1, 4, 2, 3], device=DEV)
    assert torch.equal(d(audio[perm].contiguous(), lengths[perm]), out[perm])


def test_a_hum_is_removed_as_the_reference_says():
    from efficient_tts_amd.denoise import BiasDenoiser
    from efficient_tts_amd.stft import STFTMagnitude
    n = 12345
    hum = R.hum(n)
    mag, _ = STFTMagnitude(DEV, 1024, 256, 1024)(torch.from_numpy(hum)[None].to(DEV))
    bias = mag[0, 0]
    assert np.abs(bias.cpu().numpy() - R.frame0_magnitude(hum)).max() <= 1e-4
    d = BiasDenoiser(DEV, bias, strength=1.0)
    mixed = (hum + R.signal(n, 3)).astype(np.float32)
    out = d(torch.from_numpy(np.stack([hum, mixed])).to(DEV)).cpu().numpy()
    host_bias = bias.cpu().numpy()
    for name, x, y in (("hum alone", hum, out[0]), ("hum under the signal", mixed, out[1])):
        want, got = R.level_db(R.denoise(x, host_bias, 1.0)), R.level_db(y)
        print(f"{name}: input {R.level_db(x):.2f} dB, reference {want:.3f} dB, device {got:.3f} dB")
        if x is hum:
            assert want < R.level_db(x) - 20.0                         # a denoiser that does nothing cannot pass
        assert abs(got - want) <= 0.05


def test_from_vocoder_measures_frame_0_of_the_vocoders_own_answer():
    from test_vocoder import CFG
    from efficient_tts_amd.denoise import BiasDenoiser
    from efficient_tts_amd.stft import STFTMagnitude
    from efficient_tts_amd.vocoder import HiFiGANGenerator

    def stub(mel, lens=None):
        g = torch.Generator().manual_seed(int(mel.shape[2]))
        return (torch.rand(mel.shape[0], 1, mel.shape[2] * 256, generator=g) * 0.02 - 0.01).to(mel.device) + 0.001 * float(mel[0, 0, 0])
    torch.manual_seed(0)
    gen = HiFiGANGenerator(CFG).to(DEV).eval()
    gen.remove_weight_norm()
    for vocoder, kw in ((stub, dict(frames=6, mel_value=-11.5)), (gen, dict(frames=12))):
        d = BiasDenoiser.from_vocoder(vocoder, DEV, strength=0.02, **kw)
        assert d.strength == 0.02 and d.bias.shape == (513,) and d.bias.dtype == torch.float32
        assert bool(torch.isfinite(d.bias).all()) and bool((d.bias >= 0).all()) and float(d.bias.max()) > 0
        mel = torch.full((1, 80, kw["frames"]), kw.get("mel_value", 0.0), device=DEV)
        with torch.no_grad():
            mag, _ = STFTMagnitude(DEV, 1024, 256, 1024)(vocoder(mel).reshape(1, -1).float())
        assert torch.equal(mag[0, 0].cpu(), d.bias)


def test_a_captured_call_replays_the_eager_bits_in_a_single_chain():
    audio, lengths = _batch()
    d = _denoiser()
    eager = d(audio, lengths)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        d(audio, lengths)                                              # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    # a single chain: everything the call enqueues -- the library's one launch and the few torch ops around it -- goes to the capturing stream
    # itself; nothing is forked to a side stream, so the captured graph has no parallel branches
    from efficient_tts_amd import lib as L
    lib = L.load()
    real, seen = lib.efts_denoise, []

    def spy(*args):
        seen.append((args[-1], torch.cuda.current_stream().cuda_stream, torch.cuda.is_current_stream_capturing()))
        return real(*args)
    graph = torch.cuda.CUDAGraph()
    lib.efts_denoise = spy
    try:
        with torch.cuda.graph(graph):
            captured = d(audio, lengths)
    finally:
        lib.efts_denoise = real
    assert len(seen) == 1 and seen[0][0] == seen[0][1] and seen[0][2]
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)
