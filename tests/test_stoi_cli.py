"""The command-line side of the intelligibility scores: `bin/vocoder_score.py --stoi`.  Parsing and the column and row plumbing run on the
host; one GPU case (-m gpu) scores the Griffin-Lim copy-synthesis of two tiny wav files that the test writes, with and without the flag."""
import numpy as np
import pytest

from efficient_tts_amd.bin import vocoder_score as V

BASE = ["--test_fid_scp", "t.txt", "--outdir", "o", "--vocoder", "griffinlim"]


def test_the_flag_is_off_by_default_and_changes_no_other_argument():
    plain, flagged = V.get_parser().parse_args(BASE), V.get_parser().parse_args(BASE + ["--stoi"])
    assert plain.stoi is False and flagged.stoi is True
    assert {k: v for k, v in vars(plain).items() if k != "stoi"} == {k: v for k, v in vars(flagged).items() if k != "stoi"}
    V.check_args(flagged)
    with pytest.raises(SystemExit):                                    # a switch: it takes no value
        V.get_parser().parse_args(BASE + ["--stoi=1"])


def test_rows_gain_three_columns_and_the_mean_line_two_means():
    rows = [("a", 5000, [0.1, 0.2, 0.3], [1.0, 2.0, 3.0]), ("b", 900, [0.3, 0.4, 0.5], [2.0, 3.0, 4.0])]
    before = V.format_rows(rows)[0]
    lines, _, _, s_mean, e_mean = V.format_rows(rows, stoi=[(0.75, 0.5, 31), (float("nan"), float("nan"), 3)])
    assert [line[:len(b)] for line, b in zip(lines, before)] == before
    assert [line[len(b):] for line, b in zip(lines, before)] == ["\t0.750000\t0.500000\t31", "\tnan\tnan\t3", "\t0.750000\t0.500000\t-"]
    assert (s_mean, e_mean) == (0.75, 0.5)                             # the utterance without a value is left out of the means
    lines, _, _, s_mean, e_mean = V.format_rows(rows, stoi=[(float("nan"), float("nan"), 0)] * 2)
    assert lines[-1].endswith("\tnan\tnan\t-") and np.isnan(s_mean) and np.isnan(e_mean)
    assert V.columns(stoi=True)[-3:] == list(V.STOI_COLUMNS) and V.columns(stoi=True)[:-3] == V.columns()


@pytest.mark.gpu
def test_vocoder_score_with_the_flag_appends_the_scores_and_without_it_writes_what_it_wrote(tmp_path, capsys):
    from scipy.io.wavfile import write
    rng = np.random.default_rng(3)
    (tmp_path / "wavs").mkdir()
    n = 33075                                                          # 1.5 s: 15 000 samples at 10 kHz, 116 frames
    t = np.arange(n) / 22050.0
    for k, f0 in (("a", 150.0), ("b", 210.0)):
        voice = sum(np.sin(2 * np.pi * h * f0 * t + h) / h for h in range(1, 16))
        x = 0.15 * voice * (0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t)) + 0.002 * rng.standard_normal(n)
        write(str(tmp_path / "wavs" / f"{k}.wav"), 22050, (x * 32767.0).round().astype(np.int16))
    (tmp_path / "list.txt").write_text("DUMMY/a.wav|x\nDUMMY/b.wav|y\n")
    base = ["--test_fid_scp", str(tmp_path / "list.txt"), "--wav_path", str(tmp_path / "wavs"), "--vocoder", "griffinlim", "--gl_iters", "4"]
    assert V.run_score(V.get_parser().parse_args(base + ["--outdir", str(tmp_path / "plain")])) is not None
    assert "STOI" not in capsys.readouterr().out
    V.run_score(V.get_parser().parse_args(base + ["--outdir", str(tmp_path / "stoi"), "--stoi"]))
    printed = capsys.readouterr().out
    plain, scored = (tmp_path / "plain" / "mrstft.tsv").read_text().splitlines(), (tmp_path / "stoi" / "mrstft.tsv").read_text().splitlines()
    assert len(plain) == len(scored) == 3
    assert all(len(r.split("\t")) == len(V.columns()) for r in plain)  # no such columns without the flag
    assert all(len(r.split("\t")) == len(V.columns(stoi=True)) for r in scored)
    assert ["\t".join(r.split("\t")[:len(V.columns())]) for r in scored] == plain              # the columns in front are what they were
    for r in scored[:2]:
        s, e, kept = r.split("\t")[-3:]
        assert 0.0 < float(s) <= 1.0 and 0.0 < float(e) <= 1.0 and int(kept) > 30
    s_mean, e_mean, dash = scored[2].split("\t")[-3:]
    assert dash == "-" and 0.0 < float(s_mean) <= 1.0 and 0.0 < float(e_mean) <= 1.0
    assert "mean STOI" in printed and "mean ESTOI" in printed
