"""No GPU: the host side of the sample-rate converter (efficient_tts_amd/resample.py) against the float64 restatement of
tests/resample_reference.py, the design conditions of the two filters on the reference alone, and the corpus / command-line plumbing.

Design conditions: half a second of a unit sine, the middle half of the output, the taps rounded to fp32, float64 sums.  "Lower Nyquist" is
min(src, dst) / 2, "new Nyquist" dst / 2 of a down-conversion.  A tone above the source's own Nyquist does not exist and is left out.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import resample_reference as R
from efficient_tts_amd import lib as L
from efficient_tts_amd import resample as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_PAIRS = [(48000, 22050), (44100, 22050), (24000, 22050), (16000, 22050), (22050, 48000), (22050, 16000), (22050, 8000)]
DESIGN_PAIRS = TABLE_PAIRS + [(48000, 16000), (22050, 44100)]


@pytest.mark.parametrize("quality", ["best", "fast"])
@pytest.mark.parametrize("src,dst", TABLE_PAIRS)
def test_table_equals_the_formula(src, dst, quality):
    table, Lp, M, W = S.resample_table(src, dst, quality)
    g = math.gcd(src, dst)
    Z, _, rolloff = R.QUALITIES[quality]
    assert (Lp, M) == (dst // g, src // g)
    assert W == math.ceil(Z / (rolloff * min(1.0, dst / src)))
    assert table.dtype == torch.float32 and tuple(table.shape) == (Lp, 2 * W + 1) and table.is_contiguous()
    ref = R.table(src, dst, quality)
    err = np.abs(table.numpy().astype(np.float64) - ref).max()
    print(f"{src}->{dst} {quality}: L {Lp} M {M} W {W} K {2 * W + 1}, table max abs error {err:.2e}")
    assert err <= 6e-8
    for n in (0, 1, 37, 4001, 14_700_000):
        assert S.resample_length(n, src, dst) == (n * Lp + M - 1) // M == R.length(n, src, dst)


def test_sizes_of_the_common_pairs():
    assert S.resample_table(22050, 8000, "best")[1:] == (160, 441, 187)          # K 375, the longest
    assert S.resample_table(22050, 48000, "fast")[1:] == (320, 147, 19)          # K 39, the shortest
    assert S.resample_table(16000, 22050, "best")[1:] == (441, 320, 68)
    assert S.resample_table(44100, 22050, "best")[1] == 1
    assert S.resample_length(480000, 48000, 22050) == 220500 and S.resample_length(1, 22050, 48000) == 3


def test_refusals():
    for bad in ((0, 22050), (22050, -8000), (22050.0, 16000), (22050, "16000"), (True, 16000)):
        with pytest.raises(ValueError):
            S.resample_table(*bad)
        with pytest.raises(ValueError):
            S.Resampler(None, *bad)
    with pytest.raises(ValueError):
        S.resample_table(48000, 22050, "better")
    with pytest.raises(ValueError):
        S.Resampler(None, 22050, 22050, quality="better")
    with pytest.raises(ValueError, match="MiB"):
        S.resample_table(22050, 22051)


def test_identity_and_device_only():
    r = S.Resampler(None, 22050, 22050)
    x = torch.linspace(-1, 1, 50).reshape(2, 25)
    y, n = r(x, torch.tensor([25, 7]))
    assert y is x and n.tolist() == [25, 7] and n.dtype == torch.int64
    pcm = torch.tensor([[-32768, 0, 16384]], dtype=torch.int16)
    y, n = r(pcm)
    assert y.dtype == torch.float32 and y.tolist() == [[-1.0, 0.0, 0.5]] and n.tolist() == [3]
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.Resampler(None, 48000, 22050)(torch.zeros(1, 100))
    assert S.Resampler(None, 48000, 22050).lengths_of(torch.tensor([480000, 37, 0])).tolist() == [220500, 17, 0]


def _tone(src, dst, quality, freq):
    """(output, ideal) on the middle half of half a second of sin(2 pi freq t)"""
    x = np.sin(2.0 * np.pi * freq * np.arange(src // 2) / src)
    n_out = R.length(x.shape[0], src, dst)
    n = np.arange(n_out // 4, n_out - n_out // 4)
    return R.resample(x, src, dst, quality, outputs=n, fp32_taps=True), np.sin(2.0 * np.pi * freq * n / dst)


def _db(y):
    return 20.0 * np.log10(max(np.abs(y).max(), 1e-300))


@pytest.mark.parametrize("src,dst", DESIGN_PAIRS)
def test_design_conditions_best(src, dst):
    low = min(src, dst) / 2.0
    for f in (1000.0, 0.6 * low, 0.7 * low, 0.8 * low):
        y, ideal = _tone(src, dst, "best", f)
        err = np.abs(y - ideal).max()
        print(f"best {src}->{dst}: tone {f:.0f} Hz error {err:.2e}")
        assert err <= 1e-6
    if dst < src:
        for f in (1.1 * dst / 2.0, 1.3 * dst / 2.0, 1.7 * dst / 2.0):
            if f < src / 2.0:
                level = _db(_tone(src, dst, "best", f)[0])
                print(f"best {src}->{dst}: tone {f:.0f} Hz comes out at {level:.1f} dB")
                assert level <= -130.0
        level = _db(_tone(src, dst, "best", dst / 2.0 + 50.0)[0])
        print(f"best {src}->{dst}: new Nyquist + 50 Hz comes out at {level:.1f} dB")
        assert level <= -70.0


@pytest.mark.parametrize("src,dst", DESIGN_PAIRS)
def test_design_conditions_fast(src, dst):
    low = min(src, dst) / 2.0
    for f in (1000.0, 0.6 * low, 0.7 * low):
        y, ideal = _tone(src, dst, "fast", f)
        err = np.abs(y - ideal).max()
        print(f"fast {src}->{dst}: tone {f:.0f} Hz error {err:.2e}")
        assert err <= 1e-4
    if dst < src:
        for f in (dst / 2.0 + 50.0, 1.1 * dst / 2.0, 1.3 * dst / 2.0, 1.7 * dst / 2.0):
            if f < src / 2.0:
                level = _db(_tone(src, dst, "fast", f)[0])
                print(f"fast {src}->{dst}: tone {f:.0f} Hz comes out at {level:.1f} dB")
                assert level <= -80.0


def test_dataset_source_sampling_rate(tmp_path):
    from scipy.io.wavfile import write
    from efficient_tts_amd import datasets as D
    rng = np.random.default_rng(0)
    pcm16k = rng.integers(-32768, 32767, size=1600, dtype=np.int16)
    write(str(tmp_path / "a.wav"), 16000, pcm16k)
    write(str(tmp_path / "b.wav"), 22050, pcm16k)
    (tmp_path / "phn.txt").write_text("_\nAA\nB\n")
    (tmp_path / "meta.txt").write_text("wavs/a.wav|AA B\n")
    (tmp_path / "meta_b.txt").write_text("wavs/b.wav|AA B\n")
    kw = dict(wav_path=str(tmp_path), use_phnseq=True, phnset_path=str(tmp_path / "phn.txt"))
    plain = D.TextMelLoader(str(tmp_path / "meta.txt"), **kw)
    assert plain.source_sampling_rate is None
    with pytest.raises(ValueError, match="16000 != 22050"):
        plain[0]
    ds = D.TextMelLoader(str(tmp_path / "meta.txt"), source_sampling_rate=16000, **kw)
    text, audio = ds[0]
    assert ds.source_sampling_rate == 16000 and ds.sampling_rate == 22050
    assert audio.dtype == torch.int16 and np.array_equal(audio.numpy(), pcm16k) and text.tolist() == [1, 2]
    with pytest.raises(ValueError, match="22050.*16000"):
        D.TextMelLoader(str(tmp_path / "meta_b.txt"), source_sampling_rate=16000, **kw)[0]
    assert D.TextMelLoader(str(tmp_path / "meta_b.txt"), **kw)[0][1].shape == (1600,)          # today's behaviour
    with pytest.raises(ValueError):
        D.TextMelLoader(str(tmp_path / "meta.txt"), source_sampling_rate=16000.5, **kw)


def test_parser_and_trainer_defaults():
    from efficient_tts_amd.bin import inference as I
    from efficient_tts_amd.trainer import EfficientTTSTrainer
    base = ["--checkpoint", "c.pkl", "--test_fid_scp", "t.txt", "--outdir", "o"]
    a = I.get_parser().parse_args(base)
    assert a.sampling_rate is None and a.resample_quality == "best"
    a = I.get_parser().parse_args(base + ["--sampling_rate", "16000", "--resample_quality", "fast"])
    assert a.sampling_rate == 16000 and a.resample_quality == "fast"
    cfg = dict(outdir="/tmp", log_interval_steps=5, eval_interval_steps=0, save_interval_steps=10, train_max_steps=20, grad_norm=1.0)
    t = EfficientTTSTrainer(steps=0, epochs=0, data_loader={}, sampler={}, model=torch.nn.Linear(2, 2), optimizer=None, scheduler=None, config=cfg)
    assert t.resampler is None


def test_symbols_in_header_and_binding():
    with open(os.path.join(ROOT, "include", "efts_abi.h")) as f:
        header = f.read()
    for name in ("efts_resample", "efts_resample_pcm16"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in L.exported_symbols()
        assert hasattr(L.load(), name)
