"""`python -m efficient_tts_amd.bin.score` -- mel-cepstral distortion of a checkpoint's free-running synthesis against the recordings.

    python -m efficient_tts_amd.bin.score --checkpoint exp/efts/checkpoint-100000steps.pkl --test_fid_scp test.txt --outdir exp/efts/score \\
        [--config exp/efts/config.yml] [--batch_size 16] [--precision bf16x3] [--length_scale 1.0]

Reads the `wav_path|phonemes` list of `efficient_tts_amd.bin.inference` (16-bit wav files at the front-end's rate; a path that does not
exist is looked up by its file name under dataset_params.wav_path).  Per batch, on the device: the recordings' log-mels (`LogMelFrontend`
with the recipe's frontend_params), the free-running mels (`inference_batch`), and `MelCepstralDistortion` of synthesis against recording.
Writes outdir/mcd.tsv -- utterance id, MCD in dB, frames synthesised, frames recorded, length of the warping path; the last line is the
mean -- and prints the mean.  An utterance whose synthesis has no frames has no path: its line says nan and the mean leaves it out.

The numbers compare checkpoints of this project with each other (natural-log mels of this front-end); they are not comparable to MCDs
computed from SPTK cepstra of waveforms.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

from efficient_tts_amd.bin.inference import _read_list, load_acoustic_model
from efficient_tts_amd.frontend import LogMelFrontend
from efficient_tts_amd.score import MelCepstralDistortion


def get_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="efficient_tts_amd.bin.score", description=__doc__.splitlines()[0])
    p.add_argument("--checkpoint", type=str, required=True, help="acoustic-model checkpoint (checkpoint-*steps.pkl)")
    p.add_argument("--test_fid_scp", type=str, required=True, help="utterance list: wav_path|phoneme sequence")
    p.add_argument("--outdir", type=str, required=True, help="where mcd.tsv goes")
    p.add_argument("--config", type=str, default=None, help="training config.yml (default: next to the checkpoint)")
    p.add_argument("--batch_size", type=int, default=16, help="utterances per call (default 16; every item is scored as if alone)")
    p.add_argument("--precision", type=str, default="bf16x3", choices=["bf16x3", "bf16", "fp32"], help="MFMA operand mode of the acoustic model")
    p.add_argument("--length_scale", type=float, default=1.0, help="multiplies every predicted duration (default 1.0)")
    return p


def _read_wav(path: str, wav_dir, rate: int) -> torch.Tensor:
    from scipy.io.wavfile import read
    if not os.path.exists(path) and wav_dir:
        path = os.path.join(wav_dir, os.path.basename(path))
    sr, data = read(path)
    if sr != rate or data.dtype != np.int16 or data.ndim != 1:
        raise ValueError(f"{path}: expected mono 16-bit PCM at {rate} Hz")
    return torch.from_numpy(np.ascontiguousarray(data))


def run_score(args) -> float:
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: efficient_tts_amd has no CPU path")
    if not args.length_scale > 0:
        raise ValueError("--length_scale must be > 0")
    device = torch.device("cuda")
    os.makedirs(args.outdir, exist_ok=True)
    config, phn2idx, model = load_acoustic_model(args, device)
    front = config.get("frontend_params") or {}
    frontend = LogMelFrontend(device, **front)
    rate = int(front.get("sampling_rate", 22050))
    scorer = MelCepstralDistortion(device, num_mels=frontend.n_mels)
    wav_dir = (config.get("dataset_params") or {}).get("wav_path")
    items = _read_list(args.test_fid_scp, phn2idx, with_paths=True)
    bs = max(1, int(args.batch_size))
    rows = []
    for lo in range(0, len(items), bs):
        chunk = items[lo:lo + bs]
        wavs = [_read_wav(path, wav_dir, rate) for _, _, path in chunk]
        audio = torch.nn.utils.rnn.pad_sequence(wavs, batch_first=True)
        ids = torch.nn.utils.rnn.pad_sequence([t for _, t, _ in chunk], batch_first=True)
        with torch.no_grad():
            rec, rec_len = frontend(audio, torch.tensor([w.shape[0] for w in wavs]))
            syn, syn_len = model.inference_batch(ids.to(device), torch.tensor([len(t) for _, t, _ in chunk], device=device),
                                                 length_scale=args.length_scale)[:2]
            out = scorer(syn, syn_len, rec, rec_len)
        for (utt, _, _), m, a, b, n in zip(chunk, out["mcd"].tolist(), syn_len.tolist(), rec_len.tolist(), out["path_len"].tolist()):
            rows.append((utt, m, a, b, n))
    scored = [r[1] for r in rows if np.isfinite(r[1])]
    mean = float(np.mean(scored)) if scored else float("nan")
    with open(os.path.join(args.outdir, "mcd.tsv"), "w") as handle:
        for utt, m, a, b, n in rows:
            handle.write(f"{utt}\t{m:.6f}\t{a}\t{b}\t{n}\n")
        handle.write(f"mean\t{mean:.6f}\n")
    print(f"mean MCD over {len(scored)} of {len(rows)} utterances: {mean:.4f} dB")
    return mean


def main(argv=None) -> int:
    run_score(get_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
