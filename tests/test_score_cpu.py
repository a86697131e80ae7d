"""No GPU: the host side of the scorer (efficient_tts_amd/score.py) against the float64 restatement of tests/score_reference.py, that
restatement against a brute-force enumeration of warping paths, and the plumbing: exports, command line, trainer key."""
import math
import os
import re

import numpy as np
import pytest
import torch

import score_reference as R
from efficient_tts_amd import lib as L
from efficient_tts_amd import score as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n_mels,n_coef", [(80, 13), (80, 32), (128, 24), (20, 5)])
def test_dct_table(n_mels, n_coef):
    t = S.dct_table(n_mels, n_coef)
    assert t.dtype == torch.float32 and tuple(t.shape) == (n_coef, n_mels) and t.is_contiguous()
    ref = R.table(n_mels, n_coef)
    assert np.abs(t.numpy().astype(np.float64) - ref).max() <= 2.0 ** -24 * math.sqrt(2.0 / n_mels)      # one rounding (relative 2^-24) of values up to sqrt(2 / N)
    assert np.abs(ref @ ref.T - np.eye(n_coef)).max() <= 1e-12                                          # rows are orthonormal
    # row 0 of the full DCT (the constant row, loudness) is absent: the first row is k = 1 and every row is orthogonal to a constant
    n = np.arange(n_mels)
    assert np.abs(ref[0] - math.sqrt(2.0 / n_mels) * np.cos(math.pi * (n + 0.5) / n_mels)).max() <= 1e-15
    assert np.abs(t.numpy().astype(np.float64).sum(axis=1)).max() <= 1e-5


def test_refusals_and_constant():
    assert S.MCD_DB == pytest.approx(10.0 * math.sqrt(2.0) / math.log(10.0), rel=1e-15) and R.MCD_DB == S.MCD_DB
    for bad in ((80, 0), (80, 33), (129, 13), (13, 13)):
        with pytest.raises(ValueError):
            S.dct_table(*bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.mel_cepstrum(torch.zeros(1, 4, 80), torch.tensor([4]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        S.dtw(torch.zeros(1, 4, 13), torch.tensor([4]), torch.zeros(1, 5, 13), torch.tensor([5]))
    with pytest.raises(ValueError):
        S.dtw(torch.zeros(4, 13), torch.tensor([4]), torch.zeros(1, 5, 13), torch.tensor([5]))


def _all_paths(tx, ty):
    def walk(i, j):
        if (i, j) == (tx - 1, ty - 1):
            yield [(i, j)]
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < tx and j + dj < ty:
                for rest in walk(i + di, j + dj):
                    yield [(i, j)] + rest
    return walk(0, 0)


def test_reference_dtw_equals_the_enumeration_of_all_paths():
    rng = np.random.default_rng(5)
    for tx in range(1, 6):
        for ty in range(1, 6):
            for exact in (False, True):
                x = rng.integers(-3, 4, size=(tx, 2)).astype(np.float64) if exact else rng.normal(size=(tx, 2))
                y = rng.integers(-3, 4, size=(ty, 2)).astype(np.float64) if exact else rng.normal(size=(ty, 2))
                d = np.sqrt(((x[:, None, :] - y[None, :, :]) ** 2).sum(-1))
                costs = [(sum(d[c] for c in p), len(p)) for p in _all_paths(tx, ty)]
                low = min(c for c, _ in costs)
                cost, path_len, margin = R.dtw(x, y)
                assert cost == pytest.approx(low, rel=1e-13, abs=1e-13)
                assert path_len in {n for c, n in costs if c <= low * (1 + 1e-13) + 1e-13}
                assert max(tx, ty) <= path_len <= tx + ty - 1 and margin >= 0.0


def test_reference_dtw_tie_rule():
    col = lambda *v: np.array(v, dtype=np.float64)[:, None]
    # every local cost 0: the diagonal wins every tie, the path is as short as it can be
    assert R.dtw(np.zeros((2, 3)), np.zeros((4, 3)))[:2] == (0.0, 4)
    assert R.dtw(np.zeros((5, 1)), np.zeros((5, 1)))[:2] == (0.0, 5)
    # at the last cell (i-1, j) and (i, j-1) tie at 1 below the diagonal's 3; their paths have 4 and 3 cells: (i-1, j) is tried first and stays
    cost, path_len, margin = R.dtw(col(0, 2, 0), col(0, 1, 0, 2))
    assert R.dtw(col(0, 2), col(0, 1, 0, 2))[:2] == (1.0, 4) and R.dtw(col(0, 2, 0), col(0, 1, 0))[:2] == (1.0, 3)
    assert R.dtw(col(0, 2), col(0, 1, 0))[0] == 3.0 and (cost, path_len, margin) == (3.0, 5, 0.0)
    # the mirrored pair: now (i, j-1) carries 4 cells and (i-1, j) 3, and (i-1, j) still stays
    assert R.dtw(col(0, 1, 0, 2), col(0, 2, 0))[:2] == (3.0, 4)


def test_exports_in_header_and_binding():
    with open(os.path.join(ROOT, "include", "efts_abi.h")) as f:
        header = f.read()
    for name in ("efts_mel_cepstrum", "efts_dtw"):
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert m, name
        res, args = L._SIGS[name]
        assert res is L.i32 and len(args) == len(m.group(1).split(","))
        assert name in L.exported_symbols() and hasattr(L.load(), name)
    assert "#define EFTS_ABI_VERSION 602\n" in header and L.ABI_VERSION == 602 and L.load().efts_version() == 602
    assert int(re.search(r"#define EFTS_DTW_MAX_FRAMES (\d+)", header).group(1)) >= 4096


def test_library_refuses_before_any_launch():
    lib = L.load()
    import ctypes
    buf = (ctypes.c_float * 64)()
    one = ctypes.addressof(buf)                                # a non-null address; every check precedes the launch, nothing is read
    assert lib.efts_dtw(None, 13, 0, one, 4, one, 13, 0, one, 4, 13, one, one, 1, None) == -1
    for tx, ty, d, ldx in ((8193, 4, 13, 13), (4, 8193, 13, 13), (0, 4, 13, 13), (4, 4, 33, 33), (4, 4, 0, 13), (4, 4, 13, 12)):
        assert lib.efts_dtw(one, ldx, 0, one, tx, one, 13, 0, one, ty, d, one, one, 1, None) == -2, (tx, ty, d, ldx)
    assert b"efts_dtw" in lib.efts_last_error()
    assert lib.efts_mel_cepstrum(one, 80, 0, one, None, one, 1, 4, 80, 13, None) == -1
    for n_mels, n_coef in ((129, 13), (80, 33), (0, 13), (80, 0)):
        assert lib.efts_mel_cepstrum(one, 128, 0, one, one, one, 1, 4, n_mels, n_coef, None) == -2


def test_parser_and_list_reader(tmp_path):
    from efficient_tts_amd.bin import inference as I
    from efficient_tts_amd.bin import score as C
    base = ["--checkpoint", "c.pkl", "--test_fid_scp", "t.txt", "--outdir", "o"]
    a = C.get_parser().parse_args(base)
    assert (a.config, a.batch_size, a.precision, a.length_scale) == (None, 16, "bf16x3", 1.0)
    a = C.get_parser().parse_args(base + ["--batch_size", "4", "--precision", "fp32", "--length_scale", "1.25", "--config", "x.yml"])
    assert (a.config, a.batch_size, a.precision, a.length_scale) == ("x.yml", 4, "fp32", 1.25)
    assert C._read_list is I._read_list and C.load_acoustic_model is I.load_acoustic_model           # reused, not copied
    lst = tmp_path / "t.txt"
    lst.write_text("wavs/a.wav|HH AH0\n")
    assert [(u, t.tolist(), p) for u, t, p in I._read_list(str(lst), {"HH": 0, "AH0": 1}, with_paths=True)] == [("a", [0, 1], "wavs/a.wav")]


class _Stub(torch.nn.Module):
    def forward(self, text, text_lengths, speech, speech_lengths):
        return 0.0, dict(loss=1.0, mel_loss=0.5, duration_loss=0.25)

    def inference_batch(self, *a, **k):
        raise AssertionError("the free-running pass must not run unless eval_mcd is true")


def test_trainer_key_defaults_to_off():
    from efficient_tts_amd.trainer import EfficientTTSTrainer
    cfg = dict(outdir="/tmp", log_interval_steps=5, eval_interval_steps=0, save_interval_steps=10, train_max_steps=20, grad_norm=1.0)
    batch = (torch.zeros(2, 3, dtype=torch.long), torch.tensor([3, 2]), torch.zeros(2, 5, 80), torch.tensor([5, 4]))
    for extra in ({}, {"eval_mcd": False}):
        t = EfficientTTSTrainer(steps=0, epochs=0, data_loader={"dev": [batch]}, sampler={}, model=_Stub(), optimizer=None, scheduler=None,
                                config=dict(cfg, **extra))
        seen = {}
        t._publish = seen.update
        t._evaluate()
        assert seen == {"eval/loss": 1.0, "eval/mel_loss": 0.5, "eval/dur_loss": 0.25}
