"""CPU: duration control of free-running synthesis -- the efts_duration_control export, the host-side checks of the
inference() / inference_batch() keywords (all raised before any device call) and the synthesis script's new flags."""
import pytest
import torch

from efficient_tts_amd import build as B
from efficient_tts_amd import lib as L


@pytest.fixture(scope="module")
def lib():
    B.build(verbose=False)
    return L.load()


def test_duration_control_is_exported_with_its_signature(lib):
    fn = lib.efts_duration_control
    i32, i64, vp = L.i32, L.i64, L.vp
    assert fn.restype is i32
    assert list(fn.argtypes) == [vp, i64, vp, vp, vp, i64, vp, i32, vp, vp, vp, i32, i32, vp]
    assert "efts_duration_control" in L.exported_symbols() and "efts_duration_positions" in L.exported_symbols()


def test_duration_control_argument_errors(lib):
    # rejected on the host side of the library, before any launch
    assert lib.efts_duration_control(None, 8, None, None, None, 0, None, 1, None, None, None, 2, 8, None) == -1
    with pytest.raises(ValueError):
        L.check(lib.efts_duration_control(None, 8, None, None, None, 0, None, 1, None, None, None, 2, 8, None), "efts_duration_control")


@pytest.fixture(scope="module")
def model():
    from efficient_tts_amd import EfficientTTSCNN
    return EfficientTTSCNN(num_symbols=76, dropout_rate=0.0, use_masking=True).eval()


@pytest.mark.parametrize("scale", [0.0, -1.0, float("inf"), float("nan")])
def test_bad_length_scale_is_refused(model, scale):
    text = torch.zeros(2, 8, dtype=torch.long)
    with pytest.raises(ValueError, match="length_scale"):
        model.inference(text[:1], length_scale=scale)
    with pytest.raises(ValueError, match="length_scale"):
        model.inference_batch(text, torch.tensor([8, 5]), length_scale=scale)
    with pytest.raises(ValueError, match="length_scale"):
        model.inference_batch(text, torch.tensor([8, 5]), length_scale=torch.tensor([1.0, scale]))


def test_bad_shapes_and_targets_are_refused(model):
    text = torch.zeros(2, 8, dtype=torch.long)
    tl = torch.tensor([8, 5])
    with pytest.raises(ValueError, match="length_scale"):
        model.inference_batch(text, tl, length_scale=torch.ones(3))
    with pytest.raises(ValueError, match="durations"):
        model.inference_batch(text, tl, durations=torch.ones(2, 7))
    with pytest.raises(ValueError, match="durations"):
        model.inference(text[:1], durations=torch.ones(1, 9))
    with pytest.raises(ValueError, match="target_frames"):
        model.inference_batch(text, tl, target_frames=torch.tensor([10, 0]))
    with pytest.raises(ValueError, match="target_frames"):
        model.inference(text[:1], target_frames=0)
    with pytest.raises(ValueError, match="target_frames"):
        model.inference_batch(text, tl, target_frames=torch.tensor([10]))


def test_force_delta_does_not_combine_with_a_control(model):
    text = torch.zeros(2, 8, dtype=torch.long)
    tl = torch.tensor([8, 5])
    for kw in (dict(length_scale=0.8), dict(durations=-torch.ones(2, 8)), dict(target_frames=torch.tensor([9, 9])),
               dict(return_durations=True)):
        with pytest.raises(ValueError, match="force_delta"):
            model.inference_batch(text, tl, force_delta=2.0, **kw)


def test_valid_controls_reach_the_device_check(model):
    """a well-formed control passes the host checks and then fails like any call on a box without a GPU (no CPU path)"""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(L.EftsError, match="MI355X"):          # the no-device error itself (not a TypeError for the keywords)
        model.inference(torch.zeros(1, 8, dtype=torch.long), length_scale=0.8, return_durations=True)
    with pytest.raises(L.EftsError, match="MI355X"):
        model.inference_batch(torch.zeros(2, 8, dtype=torch.long), torch.tensor([8, 5]), length_scale=torch.tensor([0.8, 1.2]),
                              durations=-torch.ones(2, 8), target_frames=torch.tensor([9, 7]), return_durations=True)


def test_controls_helper_normalises_and_keeps_the_default_path(model):
    from efficient_tts_amd import EfficientTTSCNN
    f = EfficientTTSCNN._duration_controls
    assert f(2, 8, None, None, None, False) is None
    assert f(2, 8, 1.0, None, None, False) is None                      # an explicit 1.0 is today's call
    s, o, t = f(2, 8, 0.5, None, None, False)
    assert s.tolist() == [0.5, 0.5] and o is None and t is None
    s, o, t = f(1, 4, torch.tensor(2.0), [-1, 2, 3, -1], 7, True)
    assert s.tolist() == [2.0] and o.shape == (1, 4) and o.dtype == torch.float32 and t.tolist() == [7] and t.dtype == torch.int32
    assert f(2, 8, None, None, None, True) == (None, None, None)


def test_cli_parser_accepts_the_duration_flags():
    from efficient_tts_amd.bin import inference as I
    a = I.get_parser().parse_args(["--checkpoint", "c.pkl", "--test_fid_scp", "t.txt", "--outdir", "o",
                                   "--length_scale", "0.8", "--write_durations"])
    assert a.length_scale == 0.8 and a.write_durations
    a = I.get_parser().parse_args(["--checkpoint", "c.pkl", "--test_fid_scp", "t.txt", "--outdir", "o"])
    assert a.length_scale == 1.0 and not a.write_durations


def test_durations_file_layout(tmp_path):
    from efficient_tts_amd.bin import inference as I
    p = tmp_path / "u.durations.txt"
    I._write_durations(str(p), ["HH", "AH0", "L"], [3, 0, 5], 256, 22050)
    rows = [line.split("\t") for line in p.read_text().splitlines()]
    assert [r[:4] for r in rows] == [["0", "HH", "0", "3"], ["1", "AH0", "3", "0"], ["2", "L", "3", "5"]]
    assert float(rows[2][4]) == pytest.approx(3 * 256 / 22050, abs=1e-6)
