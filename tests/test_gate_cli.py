"""GPU (-m gpu): `bin/gate.py` on three tiny wav files that the test writes -- the table, the bypass flag of a silent file, and the gated
files of --write_wavs against the module's own output after 16-bit quantisation.
"""
import numpy as np
import pytest
import torch

import gate_reference as R

pytestmark = pytest.mark.gpu


def test_gate_tsv_and_written_wavs(tmp_path):
    from scipy.io.wavfile import read, write
    from efficient_tts_amd.bin.gate import COLUMNS, main
    from efficient_tts_amd.denoise import SpectralGate
    fs = 22050
    wavs = {"burst": R.burst_item(12345, 41), "silent": np.zeros(6000, np.int16), "tail": R.tail_item(8192, 4096, 42)}
    (tmp_path / "wavs").mkdir()
    for k, v in wavs.items():
        write(str(tmp_path / "wavs" / f"{k}.wav"), fs, v)
    (tmp_path / "list.txt").write_text("".join(f"DUMMY/{k}.wav|some text\n" for k in wavs))
    assert main(["--filelist", str(tmp_path / "list.txt"), "--wav_path", str(tmp_path / "wavs"), "--outdir", str(tmp_path / "o"),
                 "--strength", "1.5", "--floor", "0.05", "--top_db", "38", "--batch_size", "2", "--write_wavs"]) == 0
    rows = [line.split("\t") for line in (tmp_path / "o" / "gate.tsv").read_text().splitlines()]
    assert tuple(rows[0]) == COLUMNS == ("id", "seconds", "frames", "noise_frames", "noise_db", "bypassed") and [r[0] for r in rows[1:]] == list(wavs)
    gate = SpectralGate("cuda", strength=1.5, floor=0.05, top_db=38.0)
    for row, (k, v) in zip(rows[1:], wavs.items()):
        ref = R.noise_profile((v.astype(np.float32) / np.float32(32768.0)), top_db=38.0)
        assert ref["margin_db"] >= 0.01                                 # the condition under which the counts must be equal
        assert float(row[1]) == pytest.approx(v.shape[0] / fs, abs=1e-4)
        assert int(row[2]) == ref["frames"] and int(row[3]) == ref["noise_frames"]
        assert int(row[5]) == int(ref["noise_frames"] < 8) == (1 if k == "silent" else 0)
        if ref["noise_frames"]:
            assert float(row[4]) == pytest.approx(ref["noise_db"], abs=1e-3)
        else:
            assert row[4] == "nan"
        out = gate(torch.from_numpy(v)[None].cuda())[0]
        sr, got = read(str(tmp_path / "o" / f"{k}.wav"))
        assert sr == fs and np.array_equal(got, torch.round(out * 32768.0).clamp(-32768, 32767).to(torch.int16).cpu().numpy())
        assert np.array_equal(got, v) == (k == "silent")                # the silent file is left as it is, the others are not
