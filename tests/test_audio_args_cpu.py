"""CPU: efficient_tts_amd/audio_args.py, the argument checks, frame counts, entry-point choice and workspace cache that the audio ops share.
No device and no library: plain values in, plain values out."""
import numpy as np
import pytest
import torch

from efficient_tts_amd import audio_args as A


def test_as_int_and_max_wav():
    for bad in (True, 1.0, "1", None, np.float32(2.0)):
        with pytest.raises(ValueError, match="hop_size must be an integer"):
            A.as_int(bad, "hop_size")
    got = A.as_int(np.int32(3), "hop_size")
    assert got == 3 and type(got) is int and A.as_int(7, "x") == 7
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_wav_value must be > 0"):
            A.max_wav(bad)
    got = A.max_wav(32768)
    assert got == 32768.0 and type(got) is float


def test_signal():
    for bad in (torch.zeros(8), torch.zeros(1, 2, 8), torch.zeros(2, 8, dtype=torch.float64), torch.zeros(2, 8, dtype=torch.int32),
                torch.zeros(0, 8), torch.zeros(2, 0, dtype=torch.int16)):
        with pytest.raises(ValueError, match="audio"):
            A.signal(bad, "audio", "Somebody")
    for ok in (torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.int16)):
        with pytest.raises(RuntimeError, match=r"Somebody runs on an MI355X device only \(no CPU path\)"):
            A.signal(ok, "audio", "Somebody")
    # a caller that moves the samples itself names nobody: the checks without the refusal, and contiguous rows
    x = torch.arange(32, dtype=torch.float32).reshape(2, 16)
    assert A.signal(x, "audio") is x
    y = A.signal(x[:, ::2], "audio")
    assert y.is_contiguous() and torch.equal(y, x[:, ::2])
    with pytest.raises(ValueError):
        A.signal(torch.zeros(8), "audio")


def test_device_lengths():
    full = A.device_lengths(None, 3, 10, "cpu")
    assert full.dtype == torch.int32 and full.tolist() == [10, 10, 10]
    for dtype in (torch.int64, torch.int32, torch.float32):
        got = A.device_lengths(torch.tensor([-3, 5, 99], dtype=dtype), 3, 10, "cpu")
        assert got.dtype == torch.int32 and got.tolist() == [0, 5, 10]
    for bad in (torch.tensor([1, 2]), torch.tensor([[1, 2, 3]]), torch.tensor(3)):
        with pytest.raises(ValueError, match=r"lengths must be \[B\]"):
            A.device_lengths(bad, 3, 10, "cpu")


@pytest.mark.parametrize("n_fft,hop", [(1024, 256), (1024, 200), (512, 512)])
def test_frame_counts_of_both_callers(n_fft, hop):
    pad = (n_fft - hop) // 2
    lens = [pad, pad + 1, 3 * hop + 1]
    lengths, n = torch.tensor(lens), 3 * hop + 1
    # the front-end: every item longer than the reflect padding, T = max frames, nothing else
    with pytest.raises(ValueError, match="longer than the reflect padding"):
        A.frame_counts(lengths, n, hop, pad)
    lh, fh, T = A.frame_counts(lengths[1:], n, hop, pad)
    assert lh == lens[1:] and fh == [(pad + 1) // hop, 3] and T == 3
    assert all(type(v) is int for v in lh + fh + [T])
    assert A.frame_counts(lengths[1:], n, hop, pad, max_frames=7) == (lens[1:], fh, 7)
    # the pitch tracker with short_ok: 0 frames for the short item, and never an empty output
    lh, fh, T = A.frame_counts(lengths, n, hop, pad, short_ok=True)
    assert lh == lens and fh == [0, (pad + 1) // hop, 3] and T == 3
    assert A.frame_counts(lengths[:1], n, hop, pad, short_ok=True) == ([pad], [0], 1)
    assert A.frame_counts(torch.tensor([0, 0]), n, hop, pad, short_ok=True) == ([0, 0], [0, 0], 1)
    assert A.frame_counts(lengths, n, hop, pad, short_ok=True, max_frames=2)[2] == 2
    for short_ok in (False, True):
        with pytest.raises(ValueError, match="max_frames must be >= 1"):
            A.frame_counts(lengths[1:], n, hop, pad, short_ok=short_ok, max_frames=0)
        with pytest.raises(ValueError, match="lengths exceed the audio buffer"):
            A.frame_counts(lengths[1:], n - 1, hop, pad, short_ok=short_ok)


def test_frame_counts_front_end_keeps_an_empty_output():
    """hop 512 of n_fft 1024: an item of pad < l < hop samples is legal and has no frame; only the pitch tracker's mode lifts T to 1"""
    assert A.frame_counts(torch.tensor([300]), 400, 512, 256) == ([300], [0], 0)
    assert A.frame_counts(torch.tensor([300]), 400, 512, 256, short_ok=True) == ([300], [0], 1)


def test_cache_evicts_by_insertion_order():
    made = []

    def make(k):
        return lambda: made.append(k) or [k]

    c = A.Cache(capacity=5)
    first = [c.get(k, make(k)) for k in range(5)]
    assert made == [0, 1, 2, 3, 4]
    assert all(c.get(k, make(k)) is first[k] for k in range(5)) and made == [0, 1, 2, 3, 4]          # a hit makes nothing
    c.get(0, make(0))                                               # ... and does not renew key 0: it is still the oldest
    c.get(5, make(5))
    assert list(c.entries) == [1, 2, 3, 4, 5] and made == [0, 1, 2, 3, 4, 5]
    assert all(c.get(k, make(k)) is first[k] for k in range(1, 5)) and made == [0, 1, 2, 3, 4, 5]   # no other key went
    assert c.get(0, make(0)) is not first[0] and list(c.entries) == [2, 3, 4, 5, 0]
    c.clear()
    assert not c.entries and c.get(2, make(2)) == [2]
    small = A.Cache(capacity=3)
    for k in "abcd":
        small.get(k, make(k))
    assert list(small.entries) == ["b", "c", "d"]
    assert A.Cache().capacity == 5


def test_pcm_entry():
    class Stub:
        efts_x = staticmethod(lambda *a: ("f32", a))
        efts_x_pcm16 = staticmethod(lambda *a: ("pcm16", a))

    fn, name, scale = A.pcm_entry(Stub, "efts_x", torch.zeros(1, 4, dtype=torch.int16), 32768.0)
    assert fn is Stub.efts_x_pcm16 and name == "efts_x_pcm16" and scale == (1.0 / 32768.0,)
    assert A.pcm_entry(Stub, "efts_x", torch.zeros(1, 4, dtype=torch.int16), 32767.0)[2] == (1.0 / 32767.0,)
    fn, name, scale = A.pcm_entry(Stub, "efts_x", torch.zeros(1, 4), 32768.0)
    assert fn is Stub.efts_x and name == "efts_x" and scale == ()
    assert fn(1, *scale, 2) == ("f32", (1, 2))
    with pytest.raises(AttributeError):
        A.pcm_entry(Stub, "efts_y", torch.zeros(1, 4), 32768.0)
