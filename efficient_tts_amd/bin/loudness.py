"""`python -m efficient_tts_amd.bin.loudness` -- how loud every recording of a corpus is, and what normalising it would do, before training on it.

    python -m efficient_tts_amd.bin.loudness --filelist train.txt --wav_path wavs --outdir exp/loudness \\
        [--target -23] [--peak_ceiling 0.99] [--batch_size 16] [--true_peak]

Reads a training file list (`audiopath|...`, one recording per line; the file name is looked up under --wav_path, 16-bit mono wav files),
runs the recordings through `efficient_tts_amd.loudness.LoudnessNormalizer` in batches -- the object that `normalize_loudness` in the
training recipe puts in front of the log-mel front-end, so --target and --peak_ceiling mean what `normalize_loudness` and
`loudness_peak_ceiling` mean there -- and writes outdir/loudness.tsv:

    id  seconds  lufs  gain_db  limited

one line per recording under a header line (lufs: the integrated loudness after ITU-R BS.1770, `-inf` for a recording without a 400 ms
block over the absolute gate; gain_db: what reaching the target takes, after the ceiling; limited: 1 when the ceiling cut the gain back),
and prints the spread.  With --true_peak every line also gets `sample_peak_db` and `true_peak_dbtp`, the largest sample and the largest value
of the 4x oversampled signal (`efficient_tts_amd.limiter.TruePeakMeter`, BS.1770 Annex 2) of the recording as it is, in dB re full scale,
`-inf` for silence.  Recordings of one batch must share one sampling rate.  There is no CPU mode.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import torch

from efficient_tts_amd.bin._io import read_wav
from efficient_tts_amd.limiter import TruePeakMeter
from efficient_tts_amd.loudness import FLAG_CEILING, FLAG_NO_LOUDNESS, LoudnessNormalizer

COLUMNS = ("id", "seconds", "lufs", "gain_db", "limited")
PEAK_COLUMNS = ("sample_peak_db", "true_peak_dbtp")


def _db(value: float) -> float:
    return 20.0 * math.log10(value) if value > 0.0 else float("-inf")


def get_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="efficient_tts_amd.bin.loudness", description=__doc__.splitlines()[0])
    p.add_argument("--filelist", type=str, required=True, help="file list: audiopath|..., one recording per line")
    p.add_argument("--wav_path", type=str, required=True, help="directory of the wav files (looked up by file name)")
    p.add_argument("--outdir", type=str, required=True, help="where loudness.tsv goes")
    p.add_argument("--target", type=float, default=-23.0, help="the integrated loudness to reach, in LUFS (default -23)")
    p.add_argument("--peak_ceiling", type=float, default=0.99, help="no sample may exceed this after the gain (default 0.99; <= 0: no ceiling)")
    p.add_argument("--batch_size", type=int, default=16, help="recordings per call (default 16; every item is treated as if alone)")
    p.add_argument("--true_peak", action="store_true", help="append sample_peak_db and true_peak_dbtp (4x oversampled) to every line")
    return p


def _read_list(path: str):
    with open(path, encoding="utf-8") as handle:
        return [line.split("|")[0].strip() for line in handle if line.strip()]


def run_loudness(args):
    if not math.isfinite(args.target):
        raise ValueError("--target must be finite")
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: efficient_tts_amd has no CPU path")
    device = torch.device("cuda")
    os.makedirs(args.outdir, exist_ok=True)
    names = _read_list(args.filelist)
    bs = max(1, int(args.batch_size))
    meters = {}                                 # one normaliser per sampling rate met
    measured = []
    peaks = TruePeakMeter(device) if args.true_peak else None
    with open(os.path.join(args.outdir, "loudness.tsv"), "w") as handle:
        handle.write("\t".join(COLUMNS + (PEAK_COLUMNS if peaks is not None else ())) + "\n")
        for lo in range(0, len(names), bs):
            chunk = names[lo:lo + bs]
            wavs, rates = zip(*(read_wav(os.path.join(args.wav_path, os.path.basename(name))) for name in chunk))
            if len(set(rates)) != 1:
                raise ValueError(f"recordings {chunk[0]} .. {chunk[-1]} have different sampling rates {sorted(set(rates))}: use --batch_size 1")
            rate = int(rates[0])
            if rate not in meters:
                meters[rate] = LoudnessNormalizer(device, rate, target_lufs=args.target,
                                                  peak_ceiling=args.peak_ceiling if args.peak_ceiling > 0 else None)
            audio = torch.nn.utils.rnn.pad_sequence(list(wavs), batch_first=True).to(device)
            _, lufs, gains, flags, _ = meters[rate](audio, torch.tensor([w.shape[0] for w in wavs]), return_stats=True)
            lufs, gains, flags = lufs.tolist(), gains.tolist(), flags.tolist()
            if peaks is not None:
                tp, sp = (v.tolist() for v in peaks(audio, torch.tensor([w.shape[0] for w in wavs])))
            for i, name in enumerate(chunk):
                utt = os.path.splitext(os.path.basename(name))[0]
                scale = meters[rate].max_wav_value if wavs[i].dtype == torch.int16 else 1.0        # the gain of int16 PCM includes 1 / max_wav_value
                gain_db = 20.0 * math.log10(gains[i] * scale)
                if not flags[i] & FLAG_NO_LOUDNESS:
                    measured.append(lufs[i])
                tail = f"\t{_db(sp[i]):.3f}\t{_db(tp[i]):.3f}" if peaks is not None else ""
                handle.write(f"{utt}\t{wavs[i].shape[0] / rate:.4f}\t{lufs[i]:.3f}\t{gain_db:.3f}\t{int(bool(flags[i] & FLAG_CEILING))}{tail}\n")
    if measured:
        print(f"{len(names)} recordings: {min(measured):.2f} .. {max(measured):.2f} LUFS, mean {sum(measured) / len(measured):.2f}; "
              f"{len(names) - len(measured)} without a loudness")
    else:
        print(f"{len(names)} recordings, none with a loudness")
    return measured


def main(argv=None) -> int:
    run_loudness(get_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
