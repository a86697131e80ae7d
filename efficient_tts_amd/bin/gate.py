"""`python -m efficient_tts_amd.bin.gate` -- what spectral gating would do to every recording of a corpus, before training on it.

    python -m efficient_tts_amd.bin.gate --filelist train.txt --wav_path wavs --outdir exp/gate \\
        [--strength 1.0] [--floor 0.1] [--top_db 40] [--min_frames 8] [--batch_size 16] [--write_wavs]

Reads a training file list (`audiopath|...`, one recording per line; the file name is looked up under --wav_path, 16-bit mono wav files),
runs the recordings through `efficient_tts_amd.denoise.SpectralGate` in batches -- the object that `denoise_corpus: true` in the training
recipe puts in front of the silence trimmer, so --strength, --floor, --top_db and --min_frames mean what `denoise_strength`, `denoise_floor`,
`denoise_top_db` and `denoise_min_frames` mean there -- and writes outdir/gate.tsv:

    id  seconds  frames  noise_frames  noise_db  bypassed

one line per recording under a header line (noise_frames: the frames more than --top_db under the loudest one, from which the profile is
taken; noise_db: their mean energy under the loudest frame's, `nan` without one; bypassed: 1 for a recording with fewer than --min_frames
of them, which is left as it is).  With --write_wavs the gated recordings go to outdir as 16-bit wav files.  There is no CPU mode.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

from efficient_tts_amd.bin._io import read_wav
from efficient_tts_amd.denoise import SpectralGate

COLUMNS = ("id", "seconds", "frames", "noise_frames", "noise_db", "bypassed")


def get_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="efficient_tts_amd.bin.gate", description=__doc__.splitlines()[0])
    p.add_argument("--filelist", type=str, required=True, help="file list: audiopath|..., one recording per line")
    p.add_argument("--wav_path", type=str, required=True, help="directory of the wav files (looked up by file name)")
    p.add_argument("--outdir", type=str, required=True, help="where gate.tsv (and the gated wav files) go")
    p.add_argument("--strength", type=float, default=1.0, help="how many times the profile is subtracted from the magnitudes (default 1.0)")
    p.add_argument("--floor", type=float, default=0.1, help="the smallest gain of a bin, 0 .. 1 (default 0.1)")
    p.add_argument("--top_db", type=float, default=40.0, help="a frame this far under the loudest one is a noise frame (default 40)")
    p.add_argument("--min_frames", type=int, default=8, help="a recording with fewer noise frames is left as it is (default 8)")
    p.add_argument("--batch_size", type=int, default=16, help="recordings per call (default 16; every item is treated as if alone)")
    p.add_argument("--write_wavs", action="store_true", help="also write the gated recordings as 16-bit wav files")
    return p


def _read_list(path: str):
    with open(path, encoding="utf-8") as handle:
        return [line.split("|")[0].strip() for line in handle if line.strip()]


def run_gate(args) -> int:
    from scipy.io.wavfile import write
    gate = SpectralGate(None, strength=args.strength, floor=args.floor, top_db=args.top_db, min_frames=args.min_frames)
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: efficient_tts_amd has no CPU path")
    device = torch.device("cuda")
    os.makedirs(args.outdir, exist_ok=True)
    names = _read_list(args.filelist)
    bs = max(1, int(args.batch_size))
    bypassed = 0
    with open(os.path.join(args.outdir, "gate.tsv"), "w") as handle:
        handle.write("\t".join(COLUMNS) + "\n")
        for lo in range(0, len(names), bs):
            chunk = names[lo:lo + bs]
            wavs, rates = zip(*(read_wav(os.path.join(args.wav_path, os.path.basename(name))) for name in chunk))
            audio = torch.nn.utils.rnn.pad_sequence(list(wavs), batch_first=True).to(device)
            out, stats = gate(audio, torch.tensor([w.shape[0] for w in wavs]), return_stats=True)
            frames, noise, level = stats["frames"].tolist(), stats["noise_frames"].tolist(), stats["noise_db"].tolist()
            pcm = torch.round(out * 32768.0).clamp(-32768, 32767).to(torch.int16).cpu().numpy() if args.write_wavs else None
            for i, name in enumerate(chunk):
                utt = os.path.splitext(os.path.basename(name))[0]
                n = int(wavs[i].shape[0])
                skip = int(noise[i] < gate.min_frames)
                bypassed += skip
                handle.write(f"{utt}\t{n / rates[i]:.4f}\t{frames[i]}\t{noise[i]}\t{level[i]:.3f}\t{skip}\n")
                if pcm is not None:
                    write(os.path.join(args.outdir, utt + ".wav"), rates[i], pcm[i, :n])
    print(f"{len(names)} recordings: {len(names) - bypassed} gated, {bypassed} left as they are")
    return bypassed


def main(argv=None) -> int:
    run_gate(get_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
