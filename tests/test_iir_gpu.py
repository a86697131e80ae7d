"""GPU (-m gpu): the IIR filter (efficient_tts_amd/iir.py, csrc/efts_iir.hip) through the Python class, and therefore the C ABI, against
the strictly sequential float64 loop in tests/iir_reference.py, which never sees the product's code.

Bound, for every element of the output: |device - reference| <= 2^-23 |reference| + 1e-10 * 0.5.  The first term is one fp32 ulp: the
reassociation of the state carry and the fma contraction move the fp64 value by parts in 1e-13 (tests/test_iir_cpu.py measures it on the
same inputs), which can flip the one rounding to fp32 and nothing more; the second term covers values near zero.  Everything else is bit
equality: int16 against its fp32 twin, an item alone and in the reversed batch, +0.0 behind every length over 1e30 garbage, a captured
call against the eager one.

Measured on an MI355X (profiles/iir_error.json): the largest error is 0.499 of the bound for every filter (2.9e-8 for the two high-passes,
4.7e-7 for de-emphasis, 3.5e-18 for pre- then de-emphasis); 1, 3, 0 and 0 of 102 266 elements are not the bits of the rounded reference.

Then the training recipe's `highpass_hz` on the trainer's staging."""
import json
import os

import numpy as np
import pytest
import torch

import iir_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
REPORT = {}


def _filters():
    from efficient_tts_amd import iir as I
    return {
        "highpass60_order2": I.highpass_sos(R.RATE, 60.0, 2),
        "highpass20_order4": I.highpass_sos(R.RATE, 20.0, 4),
        "deemphasis097": I.deemphasis_sos(0.97),
        "pre_then_deemphasis097": np.concatenate([I.preemphasis_sos(0.97), I.deemphasis_sos(0.97)]),
    }


NAMES = ("highpass60_order2", "highpass20_order4", "deemphasis097", "pre_then_deemphasis097")


def _filter(name):
    from efficient_tts_amd.iir import IIRFilter
    return IIRFilter(DEV, _filters()[name])


def _inputs(pcm16=False):
    audio, lengths = R.batch(pcm16)
    return torch.from_numpy(audio.copy()).to(DEV), torch.from_numpy(lengths.copy()).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _record(name, entry):
    REPORT[name] = entry
    if os.environ.get("EFTS_WRITE_PROFILES"):                          # how profiles/iir_error.json is produced
        with open(os.path.join(ROOT, "profiles", "iir_error.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
            f.write("\n")


@pytest.fixture(scope="module")
def outputs():
    """the device output of the fp32 batch per filter, computed once"""
    audio, lengths = _inputs()
    return {name: _filter(name)(audio, lengths) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_output_against_the_sequential_float64_reference(name, outputs):
    out = outputs[name]
    assert out.dtype == torch.float32 and out.shape == (len(R.LENGTHS), R.N)
    o = out.cpu().numpy()
    ref = R.reference(_filters()[name])
    worst, worst_ratio, unequal, total = 0.0, 0.0, 0, 0
    for b, n in enumerate(R.LENGTHS):
        err = np.abs(o[b, :n].astype(np.float64) - ref[b])
        if n:
            worst = max(worst, float(err.max()))
            worst_ratio = max(worst_ratio, float((err / R.bound(ref[b])).max()))
        unequal += int(np.count_nonzero(o[b, :n] != ref[b].astype(np.float32)))
        total += n
    print(f"{name}: max |device - reference| = {worst:.3e}, at most {worst_ratio:.3f} of the bound; {unequal} of {total} elements are not the "
          f"rounded reference")
    _record(name, {"max_abs_error": worst, "max_error_over_bound": worst_ratio, "elements_not_bit_equal_to_rounded_reference": unequal,
                   "elements": total})
    for b, n in enumerate(R.LENGTHS):
        assert np.all(np.abs(o[b, :n].astype(np.float64) - ref[b]) <= R.bound(ref[b])), (name, b)


@pytest.mark.parametrize("name", NAMES)
def test_zero_behind_every_length_over_garbage(name, outputs):
    audio, _ = _inputs()
    for b, n in enumerate(R.LENGTHS):
        assert n == R.N or float(audio[b, n]) == float(np.float32(R.GARBAGE))
        assert not _bits(outputs[name][b, n:]).any(), (name, b)
    assert not _bits(outputs[name][0]).any()                           # the empty item


@pytest.mark.parametrize("name", NAMES)
def test_int16_gives_the_bits_of_its_fp32_twin(name):
    pcm, lengths = _inputs(True)
    twin = torch.from_numpy(R.twin(R.batch(True)[0])).to(DEV)
    f = _filter(name)
    assert torch.equal(_bits(f(pcm, lengths)), _bits(f(twin, lengths)))


@pytest.mark.parametrize("name", NAMES)
def test_an_item_alone_and_in_the_reversed_batch_has_the_bits_of_the_batch(name, outputs):
    audio, lengths = _inputs()
    f = _filter(name)
    for b, n in enumerate(R.LENGTHS):
        alone = f(audio[b:b + 1, :max(n, 1)].contiguous(), lengths[b:b + 1])
        assert torch.equal(_bits(alone[0, :n]), _bits(outputs[name][b, :n])), (name, b)
    back = f(audio.flip(0).contiguous(), lengths.flip(0))
    assert torch.equal(_bits(back.flip(0)), _bits(outputs[name]))


def test_preemphasis_then_deemphasis_returns_the_input(outputs):
    """the carry error detector: a wrong start state of one segment shows as an error of order 1e-2"""
    audio, _ = _inputs()
    o, x = outputs["pre_then_deemphasis097"].cpu().numpy(), audio.cpu().numpy()
    for b, n in enumerate(R.LENGTHS):
        want = x[b, :n].astype(np.float64)
        assert np.all(np.abs(o[b, :n].astype(np.float64) - want) <= R.bound(want)), b


def test_a_captured_call_replays_the_eager_bits(outputs):
    name = "highpass20_order4"
    audio, lengths = _inputs()
    f = _filter(name)
    static_audio = torch.zeros_like(audio)
    f(static_audio, lengths)                                           # workspace and matrices allocated outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = f(static_audio, lengths)
    static_audio.copy_(audio)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(static_out), _bits(outputs[name]))
        static_out.zero_()


# ---------------------------------------------------------------------------------------------- the training recipe
def _trainer():
    from efficient_tts_amd.frontend import LogMelFrontend
    from efficient_tts_amd.trainer import EfficientTTSTrainer
    cfg = dict(outdir="/tmp", log_interval_steps=5, eval_interval_steps=0, save_interval_steps=10, train_max_steps=20, grad_norm=1.0,
               bucket_frames=0, bucket_phones=0)
    t = EfficientTTSTrainer(steps=0, epochs=0, data_loader={}, sampler={}, model=torch.nn.Linear(2, 2), optimizer=None, scheduler=None, config=cfg,
                            device=torch.device(DEV))
    t.frontend = LogMelFrontend(DEV)
    return t


def test_highpass_hz_in_the_trainers_staging():
    from efficient_tts_amd.bin.train import build_highpass, build_preemphasis
    from efficient_tts_amd.datasets import SyntheticTextAudio, TextMelCollate
    batch = TextMelCollate()([(text, audio) for text, audio in SyntheticTextAudio(n_items=3, min_phones=6, max_phones=12)])
    text, text_lengths, audio, lengths = batch
    t = _trainer()
    assert t.highpass is None and t.preemphasis is None and build_highpass({}, DEV) is None and build_preemphasis({}, DEV) is None
    plain = t._stage(batch)                                            # the attributes left None: the path of every recipe without the keys
    want, want_lengths = t.frontend(audio.to(DEV), lengths.to(DEV))
    assert torch.equal(_bits(plain[2]), _bits(want)) and torch.equal(plain[3], want_lengths)
    for attr, build, cfg in (("highpass", build_highpass, {"highpass_hz": 60}), ("highpass", build_highpass, {"highpass_hz": 20, "highpass_order": 4}),
                             ("preemphasis", build_preemphasis, {"preemphasis": 0.97})):
        t = _trainer()
        f = build(cfg, DEV)
        setattr(t, attr, f)
        with_key = t._stage(batch)
        by_hand = _trainer()._stage((text, text_lengths, f(audio.to(DEV), lengths.to(DEV)), lengths))
        assert not torch.equal(with_key[2], plain[2]), cfg
        assert torch.equal(_bits(with_key[2]), _bits(by_hand[2])) and torch.equal(with_key[3], by_hand[3]), cfg
