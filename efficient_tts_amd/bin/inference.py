"""`python -m efficient_tts_amd.bin.inference` -- text (phoneme sequences) to 16-bit wav files on MI355X.

Takes the reference synthesis script's command line (nntts/bin/inference.py:128-176):

    python -m efficient_tts_amd.bin.inference --checkpoint exp/efts/checkpoint-100000steps.pkl --test_fid_scp test.txt \\
        --outdir exp/efts/wav [--config exp/efts/config.yml] [--verbose 1]

and runs the whole chain on the GPU: `EfficientTTSCNN.inference` (free-running acoustic model) followed by the
HiFi-GAN V1 generator (efficient_tts_amd.vocoder).  Differences from the reference script:
  * the vocoder weights are named explicitly (`--vocoder_config`, `--vocoder_checkpoint`): the reference hard-codes
    a checkpoint that is not part of its repository; without one the generator runs with random weights and says so
    (useful for smoke tests and timing only), `--no_vocoder` writes the mel-spectrograms as .npy instead;
  * `--vocoder griffinlim [--gl_iters N]` replaces the generator by Griffin-Lim phase reconstruction on the device
    (efficient_tts_amd.griffinlim): no vocoder checkpoint is read, the audio is intelligible but not HiFi-GAN quality;
  * `--batch_size N` synthesises N utterances per call with `inference_batch` (each item equals its B = 1 result);
  * every line of the list is processed (the reference stops after 10), alignment plots are not drawn;
  * RTF is reported as the reference does (wall time of model + vocoder over audio duration), synchronised per call;
  * `--length_scale S` multiplies every predicted duration (> 1: slower speech), `--write_durations` writes the frames per
    phoneme next to each output (<id>_<step>.durations.txt: index, phoneme, start frame, frames, start time in seconds);
  * `--sampling_rate R [--resample_quality best|fast]` writes the wav files at R Hz instead of the vocoder's 22 050 Hz: the vocoder's
    output is converted on the device (efficient_tts_amd.resample) in front of the 16-bit quantisation;
  * `--write_f0` writes the pitch contour of every utterance next to its wav (<id>_<step>.f0.txt: frame index, time in seconds, f0 in Hz with 0 for an
    unvoiced frame), tracked on the device from the vocoder's output (efficient_tts_amd.pitch) on the mel frames' grid;
    `--f0_smooth` decides the frames of an utterance together (the tracker's Viterbi path over all lags) instead of one by one;
  * `--loudness L [--loudness_peak_ceiling 0.99]` brings every utterance to an integrated loudness of L LUFS (ITU-R BS.1770, for example -23)
    on the device (efficient_tts_amd.loudness), behind the vocoder and in front of the optional rate conversion; a gain that would take the
    peak over the ceiling is cut back.  Without the flag the wav files are byte for byte what they were;
  * `--denoise S` (S > 0, for example 0.01) removes the vocoder's bias noise on the device (efficient_tts_amd.denoise): the magnitude spectrum
    of the vocoder's answer to a blank mel is measured once after the vocoder is built, and S times it is subtracted from every frame of
    every utterance (1024-point STFT, hop 256, phases kept) -- behind the vocoder, in front of `--loudness` and `--sampling_rate`;
    `--write_f0` then tracks the denoised signal.  Without the flag the wav files are byte for byte what they were;
  * `--limit_true_peak DBTP` (at most 0, for example -1) holds every utterance under that true-peak ceiling on the device
    (efficient_tts_amd.limiter): a look-ahead limiter built for the OUTPUT rate, the last step in front of the 16-bit quantisation, behind
    `--sampling_rate`, so it sees the samples that are written.  Together with `--loudness` the normaliser runs without its own ceiling --
    the target is reached and the limiter takes the peaks -- and an explicit `--loudness_peak_ceiling` is refused.  Without the flag the
    wav files are byte for byte what they were;
  * `--use_ema` loads the averaged weights of the checkpoint (its "ema" entry: a run with `ema_decay` in its YAML writes one,
    efficient_tts_amd.ema) instead of the raw ones; a checkpoint without that entry is refused at start-up.  Without the flag every byte
    written is what it was.
"""
from __future__ import annotations

import argparse
import logging
import math
import os
import sys
import time
from typing import List, Tuple

import numpy as np
import torch
import yaml

from efficient_tts_amd import models
from efficient_tts_amd.denoise import BiasDenoiser
from efficient_tts_amd.griffinlim import GriffinLimVocoder
from efficient_tts_amd.limiter import PeakLimiter
from efficient_tts_amd.iir import build_chain
from efficient_tts_amd.loudness import LoudnessNormalizer
from efficient_tts_amd.pitch import PitchTracker
from efficient_tts_amd.resample import QUALITIES, Resampler
from efficient_tts_amd.vocoder import HiFiGANGenerator, load_hifigan_generator

HOP = 256             # samples per mel frame of the acoustic model's and the front-end's frames, and so of every vocoder here
_V1 = dict(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
           resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80)
SAMPLING_RATE = 22050


class _Explicit(argparse.Action):
    """stores the value and notes that the argument was given, so that its default can be told from the same value spelled out"""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        setattr(namespace, self.dest + "_given", True)


def get_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="efficient_tts_amd.bin.inference", description=__doc__.splitlines()[0])
    p.add_argument("--checkpoint", type=str, required=True, help="acoustic-model checkpoint (checkpoint-*steps.pkl)")
    p.add_argument("--test_fid_scp", type=str, required=True, help="utterance list: wav_path|phoneme sequence")
    p.add_argument("--outdir", type=str, required=True, help="where the generated speech goes")
    p.add_argument("--config", type=str, default=None, help="training config.yml (default: next to the checkpoint)")
    p.add_argument("--vocoder_config", type=str, default=None, help="HiFi-GAN config.json (default: the V1 LJSpeech configuration); with gen_istft_n_fft / gen_istft_hop_size an iSTFTNet one, e.g. C8C8I: upsample_rates [8, 8], upsample_kernel_sizes [16, 16], gen_istft_n_fft 16, gen_istft_hop_size 4")
    p.add_argument("--vocoder_checkpoint", type=str, default=None, help='HiFi-GAN checkpoint with a "generator" state_dict')
    p.add_argument("--vocoder", type=str, default="hifigan", choices=["hifigan", "griffinlim"],
                   help="hifigan (default): the HiFi-GAN V1 generator; griffinlim: phase reconstruction on the device, needs no vocoder checkpoint")
    p.add_argument("--gl_iters", type=int, default=32, help="Griffin-Lim iterations (--vocoder griffinlim; default 32)")
    p.add_argument("--no_vocoder", action="store_true", help="write <id>_<step>.npy mel-spectrograms instead of wav files")
    p.add_argument("--batch_size", type=int, default=1, help="utterances per acoustic-model call (default 1, as the reference)")
    p.add_argument("--precision", type=str, default="bf16x3", choices=["bf16x3", "bf16", "fp32"],
                   help="MFMA operand mode of the acoustic model and the vocoder (fp32: exact fp32 operands, the reference-parity mode)")
    p.add_argument("--length_scale", type=float, default=1.0, help="multiplies every predicted duration (default 1.0; > 1: slower speech)")
    p.add_argument("--write_durations", action="store_true",
                   help="also write <id>_<step>.durations.txt: token index, phoneme, start frame, frame count, start time in seconds")
    p.add_argument("--sampling_rate", type=int, default=None,
                   help=f"sampling rate of the written wav files in Hz (default: the vocoder's, {SAMPLING_RATE}); other rates are converted on the device")
    p.add_argument("--resample_quality", type=str, default="best", choices=sorted(QUALITIES), help="filter of --sampling_rate (default best)")
    p.add_argument("--write_f0", action="store_true",
                   help="also write <id>_<step>.f0.txt: frame index, time in seconds, f0 in Hz (0: unvoiced) of the vocoder's output")
    p.add_argument("--f0_smooth", action="store_true", help="--write_f0: smooth the contour across frames (the cheapest path over the lags of all frames)")
    p.add_argument("--loudness", type=float, default=None,
                   help="bring every utterance to this integrated loudness in LUFS (ITU-R BS.1770), for example -23 (default: leave the level)")
    p.add_argument("--loudness_peak_ceiling", type=float, default=0.99, action=_Explicit,
                   help="--loudness: no sample may exceed this (default 0.99; <= 0: no ceiling; not together with --limit_true_peak)")
    p.add_argument("--limit_true_peak", type=float, default=None,
                   help="hold every utterance under this true-peak ceiling in dBTP, for example -1 (default: no limiter)")
    p.add_argument("--denoise", type=float, default=None,
                   help="subtract this many times the vocoder's bias spectrum from every frame's magnitudes, for example 0.01 (default: no denoiser)")
    p.add_argument("--highpass_hz", type=float, default=None,
                   help="run a Butterworth high-pass at this cutoff over the vocoder's output, for example 60 (default: no filter)")
    p.add_argument("--highpass_order", type=int, default=None, help="--highpass_hz: 2 (default) or 4")
    p.add_argument("--deemphasis", type=float, default=None,
                   help="undo a pre-emphasis of this coefficient on the vocoder's output, for example 0.97, behind --highpass_hz (default: none)")
    p.add_argument("--use_ema", action="store_true", help=USE_EMA_HELP)
    p.add_argument("--verbose", type=int, default=1)
    return p


def _read_list(path: str, phn2idx, with_paths: bool = False) -> List[Tuple[str, torch.Tensor]]:
    """(utterance id, phoneme ids) per line of a `wav_path|phonemes` list; with_paths: (utterance id, phoneme ids, wav_path)"""
    items = []
    with open(path) as handle:
        for line in handle:
            line = line.strip()
            if not line:
                continue
            wav_path, text = line.split("|")[:2]
            utt = os.path.splitext(os.path.basename(wav_path))[0]
            ids = torch.tensor([phn2idx[p] for p in text.split()], dtype=torch.long)
            items.append((utt, ids, wav_path) if with_paths else (utt, ids))
    return items


USE_EMA_HELP = 'synthesise with the averaged weights of the checkpoint (its "ema" entry, written by a run with ema_decay) instead of the raw ones'


def averaged_weights(state: dict, path: str = "the checkpoint") -> dict:
    """--use_ema: the "model" entry of a checkpoint's "ema" entry; a checkpoint without one is refused"""
    ema = state.get("ema")
    if not isinstance(ema, dict) or "model" not in ema:
        raise ValueError(f'--use_ema: {path} holds no "ema" entry: it was trained without `ema_decay` in its YAML (for example ema_decay: 0.999), '
                         f"so there are no averaged weights to load")
    return ema["model"]


def load_acoustic_model(args, device):
    """(config, phn2idx, model) of --checkpoint / --config / --precision [/ --use_ema]: the model in eval mode, weight norm removed"""
    config_path = args.config or os.path.join(os.path.dirname(args.checkpoint), "config.yml")
    with open(config_path) as handle:
        config = yaml.safe_load(handle)
    data_params = config.get("dataset_params") or {}
    if not data_params.get("use_phnseq", False):
        raise NotImplementedError("only phoneme-sequence recipes (dataset_params.use_phnseq: true) are supported")
    with open(data_params["phnset_path"]) as handle:
        phn2idx = {p.strip(): i for i, p in enumerate(handle)}
    model = getattr(models, config["model_name"])(precision=args.precision, **config["model_params"])
    state = torch.load(args.checkpoint, map_location="cpu")
    model.load_state_dict(averaged_weights(state, args.checkpoint) if getattr(args, "use_ema", False) else state["model"])
    model = model.to(device).eval()
    model.remove_weight_norm()
    return config, phn2idx, model


def build_vocoder(args, device):
    """the vocoder of --vocoder / --vocoder_config / --vocoder_checkpoint / --gl_iters / --precision (shared with efficient_tts_amd.bin.score)"""
    if args.vocoder == "griffinlim":
        return GriffinLimVocoder(device, n_iter=args.gl_iters, precision="fp32" if args.precision == "fp32" else "bf16x3")
    if args.vocoder_checkpoint:
        if not args.vocoder_config:
            raise ValueError("--vocoder_checkpoint needs --vocoder_config")
        vocoder = load_hifigan_generator(device, args.vocoder_config, args.vocoder_checkpoint, precision=args.precision)
        if vocoder.hop != HOP:                  # (an iSTFTNet config counts its head's hop in: C8C8I is 8 * 8 * 4 = 256)
            raise ValueError(f"--vocoder_config: the generator makes {vocoder.hop} samples per mel frame; the mel frames here are {HOP} samples at "
                             f"{SAMPLING_RATE} Hz (upsample_rates, times gen_istft_hop_size for an iSTFT head, must multiply to {HOP})")
        return vocoder
    logging.warning("no --vocoder_checkpoint: the HiFi-GAN generator runs with RANDOM weights (timing / smoke only)")
    vocoder = HiFiGANGenerator(_V1, precision=args.precision).to(device).eval()
    vocoder.remove_weight_norm()
    return vocoder


def _write_f0(path: str, f0, hop: int, sampling_rate: int) -> None:
    with open(path, "w") as handle:
        for t, f in enumerate(f0):
            handle.write(f"{t}\t{t * hop / sampling_rate:.6f}\t{f:.3f}\n")


def _write_wav(path: str, samples: torch.Tensor, sampling_rate: int = SAMPLING_RATE) -> None:
    from scipy.io.wavfile import write
    pcm = (samples.clamp(-1.0, 1.0) * 32767.0).round().to(torch.int16).cpu().numpy()
    write(path, sampling_rate, pcm)


def _write_durations(path: str, phonemes: List[str], frames, hop: int, sampling_rate: int) -> None:
    start = 0
    with open(path, "w") as handle:
        for i, (p, n) in enumerate(zip(phonemes, frames)):
            handle.write(f"{i}\t{p}\t{start}\t{int(n)}\t{start * hop / sampling_rate:.6f}\n")
            start += int(n)


def check_f0_smooth(args) -> None:
    """--f0_smooth changes how --write_f0 tracks: alone it would do nothing, so it is refused (on the host, before anything is loaded)"""
    if args.f0_smooth and not args.write_f0:
        raise ValueError("--f0_smooth smooths the contour that --write_f0 writes: give --write_f0 as well")


def build_loudness(args, device=None):
    """the LoudnessNormalizer for the vocoder's output, or None without --loudness (checked on the host, before anything is loaded)"""
    if args.loudness is None:
        return None
    if args.no_vocoder:
        raise ValueError("--loudness sets the level of the vocoder's output: it cannot be combined with --no_vocoder")
    ceiling = args.loudness_peak_ceiling
    if getattr(args, "limit_true_peak", None) is not None:       # the limiter behind it takes the peaks: the target is reached
        ceiling = 0.0
    return LoudnessNormalizer(device, SAMPLING_RATE, target_lufs=args.loudness, peak_ceiling=ceiling if ceiling > 0 else None)


def build_limiter(args, out_rate: int = SAMPLING_RATE, device=None):
    """the PeakLimiter for the samples that are written, at their rate, or None without --limit_true_peak (checked on the host, before
    anything is loaded)"""
    if args.limit_true_peak is None:
        return None
    if args.no_vocoder:
        raise ValueError("--limit_true_peak limits the vocoder's output: it cannot be combined with --no_vocoder")
    if not (math.isfinite(args.limit_true_peak) and args.limit_true_peak <= 0.0):
        raise ValueError("--limit_true_peak must be a finite ceiling of at most 0 dBTP, for example -1")
    if getattr(args, "loudness_peak_ceiling_given", False):
        raise ValueError("--limit_true_peak takes the peaks behind --loudness, which then runs without a ceiling of its own: "
                         "leave --loudness_peak_ceiling out")
    return PeakLimiter(device, int(out_rate), ceiling_dbtp=args.limit_true_peak)


def build_filter(args, device=None):
    """the IIRFilter for the vocoder's output -- the high-pass of --highpass_hz, then the de-emphasis of --deemphasis -- or None without
    either (checked on the host, before anything is loaded)"""
    hz, order, coef = getattr(args, "highpass_hz", None), getattr(args, "highpass_order", None), getattr(args, "deemphasis", None)
    if hz is None and order is None and coef is None:
        return None
    if args.no_vocoder:
        raise ValueError("--highpass_hz and --deemphasis filter the vocoder's output: they cannot be combined with --no_vocoder")
    return build_chain(device, SAMPLING_RATE, hz, order, coef)


def build_denoiser(args, vocoder=None, device=None):
    """the BiasDenoiser for the vocoder's output, its bias measured from `vocoder`, or None without --denoise.  Without a vocoder: only the
    checks (on the host, before anything is loaded)"""
    if args.denoise is None:
        return None
    if args.no_vocoder:
        raise ValueError("--denoise cleans the vocoder's output: it cannot be combined with --no_vocoder")
    if not (args.denoise > 0 and math.isfinite(args.denoise)):
        raise ValueError("--denoise must be a finite strength > 0 (leave the flag out for no denoiser)")
    if vocoder is None:
        return None
    return BiasDenoiser.from_vocoder(vocoder, device, strength=args.denoise)


def run_tts(args) -> float:
    check_f0_smooth(args)
    build_loudness(args)
    build_denoiser(args)
    build_filter(args)
    build_limiter(args, SAMPLING_RATE if args.sampling_rate is None else int(args.sampling_rate))
    level = {0: logging.WARNING, 1: logging.INFO}.get(args.verbose, logging.DEBUG)
    logging.basicConfig(level=level, stream=sys.stdout, force=True, format="%(asctime)s %(levelname)s %(name)s:%(lineno)d  %(message)s")
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: efficient_tts_amd has no CPU path")
    device = torch.device("cuda")
    os.makedirs(args.outdir, exist_ok=True)
    config, phn2idx, model = load_acoustic_model(args, device)
    idx2phn = {i: p for p, i in phn2idx.items()}
    hop = int(config.get("hop_size", 256))
    sampling_rate = int(config.get("sampling_rate", SAMPLING_RATE))
    if not args.length_scale > 0:
        raise ValueError("--length_scale must be > 0")
    out_rate = SAMPLING_RATE if args.sampling_rate is None else int(args.sampling_rate)
    if out_rate <= 0:
        raise ValueError("--sampling_rate must be > 0")
    ctl = dict(length_scale=args.length_scale, return_durations=args.write_durations)
    items = _read_list(args.test_fid_scp, phn2idx)
    logging.info(f"{len(items)} utterances to synthesise")
    step = os.path.basename(args.checkpoint).split("-")[-1][:-4]

    if args.write_f0 and args.no_vocoder:
        raise ValueError("--write_f0 tracks the vocoder's output: it cannot be combined with --no_vocoder")
    vocoder = None if args.no_vocoder else build_vocoder(args, device)
    tracker = PitchTracker(device, sampling_rate=SAMPLING_RATE, n_fft=1024, hop_size=256, smooth=args.f0_smooth) if args.write_f0 else None
    denoiser = build_denoiser(args, vocoder, device)
    iir = build_filter(args, device)
    loudness = build_loudness(args, device)
    resampler = None
    if vocoder is not None and out_rate != SAMPLING_RATE:
        resampler = Resampler(device, SAMPLING_RATE, out_rate, quality=args.resample_quality)
    limiter = build_limiter(args, out_rate, device)

    total_rtf, done = 0.0, 0
    bs = max(1, int(args.batch_size))
    for lo in range(0, len(items), bs):
        chunk = items[lo:lo + bs]
        torch.cuda.synchronize()
        start = time.perf_counter()
        with torch.no_grad():
            if len(chunk) == 1:
                out = model.inference(chunk[0][1][None].to(device), **ctl)
                mels = [out[0][0]]
                frames = [out[2][0]] if args.write_durations else None
            else:
                lens = torch.tensor([len(t) for _, t in chunk])
                ids = torch.zeros(len(chunk), int(lens.max()), dtype=torch.long)
                for n, (_, t) in enumerate(chunk):
                    ids[n, :len(t)] = t
                out = model.inference_batch(ids.to(device), lens.to(device), **ctl)
                mel, mel_lens = out[0], out[1]
                mels = [mel[n, :int(mel_lens[n])] for n in range(len(chunk))]
                frames = [out[3][n, :int(lens[n])] for n in range(len(chunk))] if args.write_durations else None
            if vocoder is None:
                outs = mels
            elif len(chunk) == 1:
                outs = raw = [vocoder(mels[0].t()[None].contiguous())[0, 0]]
                if denoiser is not None:
                    outs = raw = [denoiser(outs[0][None].float())[0]]
                if iir is not None:
                    outs = [iir(outs[0][None].float())[0]]
                if loudness is not None:
                    outs = [loudness(outs[0][None].float())[0]]
                if resampler is not None:
                    outs = [resampler(outs[0][None].float())[0][0]]
                if limiter is not None:
                    outs = [limiter(outs[0][None].float())[0]]
            else:                                       # one batched generator pass; every item equals its single-utterance result
                audio = vocoder(mel.transpose(1, 2).contiguous(), mel_lens)
                if denoiser is not None:                # ragged: every item is framed and reflected at its own ends
                    audio = denoiser(audio[:, 0].float(), mel_lens.to(audio.device) * 256)[:, None]
                raw = [audio[n, 0, :int(mel_lens[n]) * 256] for n in range(len(chunk))]
                if iir is not None:                     # ragged: every item is filtered from zero state over its own samples
                    audio = iir(audio[:, 0].float(), mel_lens.to(audio.device) * 256)[:, None]
                if loudness is not None:                # ragged as well: every item is measured over its own samples only
                    audio = loudness(audio[:, 0].float(), mel_lens.to(audio.device) * 256)[:, None]
                if resampler is None:
                    outs = [audio[n, 0, :int(mel_lens[n]) * 256] for n in range(len(chunk))]
                else:                                   # ragged: every item is converted from its own samples only
                    audio, audio_lens = resampler(audio[:, 0].float(), mel_lens.to(audio.device) * 256)
                    outs = [audio[n, :int(audio_lens[n])] for n in range(len(chunk))]
                if limiter is not None:                 # the last step, on the samples that are written; ragged like the others
                    lens_out = torch.tensor([o.shape[0] for o in outs], device=audio.device)
                    limited = limiter(torch.nn.utils.rnn.pad_sequence([o.float() for o in outs], batch_first=True), lens_out)
                    outs = [limited[n, :o.shape[0]] for n, o in enumerate(outs)]
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - start
        seconds = sum(m.shape[0] for m in mels) * 256 / SAMPLING_RATE
        total_rtf += elapsed / seconds * len(chunk)
        done += len(chunk)
        for (utt, _), out in zip(chunk, outs):
            if vocoder is None:
                np.save(os.path.join(args.outdir, f"{utt}_{step}.npy"), out.cpu().numpy())
            else:
                _write_wav(os.path.join(args.outdir, f"{utt}_{step}.wav"), out, out_rate)
        if tracker is not None:                         # outside the timed span: the contour of the vocoder's own output, before any rate conversion
            for (utt, _), wav in zip(chunk, raw):
                with torch.no_grad():
                    f0, _, n = tracker(wav[None].float(), torch.tensor([wav.shape[0]]), short_ok=True)
                _write_f0(os.path.join(args.outdir, f"{utt}_{step}.f0.txt"), f0[0, :int(n[0])].cpu().tolist(), 256, SAMPLING_RATE)
        if frames is not None:
            for (utt, ids1), fr in zip(chunk, frames):
                _write_durations(os.path.join(args.outdir, f"{utt}_{step}.durations.txt"), [idx2phn[int(i)] for i in ids1],
                                 fr.cpu().tolist(), hop, sampling_rate)
        logging.debug(f"{[u for u, _ in chunk]}: {elapsed * 1e3:.2f} ms for {seconds:.2f} s of audio")
    rtf = total_rtf / max(done, 1)
    logging.info(f"Finished generation of {done} utterances (RTF = {rtf:.05f}).")
    return rtf


def main(argv=None) -> int:
    run_tts(get_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
