"""Datasets / collate of the reference recipe, re-cut for a device-side feature pipeline.

Name-lookup namespace mirroring ``nntts.datasets`` (reference nntts/bin/train.py:108-137):
``getattr(efficient_tts_amd.datasets, config["dataset_type"])(meta_file=..., **config["dataset_params"])``.

Difference from the reference by design: `TextMelLoader` (nntts/datasets/taco2_data.py:17-95) computes the
mel-spectrogram of every item on a CPU dataloader worker, every epoch.  Here the dataset yields the raw
int16 waveform and `TextMelCollate` pads WAVEFORMS; the trainer turns the padded batch into
(mel, mel_lengths) on the GPU with `efficient_tts_amd.frontend.LogMelFrontend` (one batched launch chain).
Batch layout otherwise as the reference's collate (:95-139): items sorted by decreasing text length, text
right-padded with 0, lengths as LongTensors.
"""
from __future__ import annotations

import os
import random
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.utils.data


def load_filepaths_and_text(filename: str, split: str = "|") -> List[List[str]]:
    with open(filename, encoding="utf-8") as f:
        return [line.strip().split(split) for line in f if line.strip()]


class TextMelLoader(torch.utils.data.Dataset):
    """(phoneme ids, int16 waveform) pairs from an `audiopath|phoneme sequence` file list.

    Same constructor arguments as the reference class (taco2_data.py:23-45), plus `source_sampling_rate`: the rate the files are
    recorded at when it is not `sampling_rate` (None: they must be at `sampling_rate`).  Only the phoneme-sequence
    input of the published recipe is supported (`use_phnseq: True` in egs/lj/conf/*.yaml); the grapheme
    path needs the reference's text cleaners (nntts/text), which are outside this package's scope."""

    def __init__(self, meta_file: str, text_cleaners: Sequence[str] = ("english_cleaners",), max_wav_value: float = 32768.0,
                 sampling_rate: int = 22050, wav_path: str = "", use_phnseq: bool = False, phnset_path: Optional[str] = None,
                 source_sampling_rate: Optional[int] = None):
        if not use_phnseq:
            raise NotImplementedError("only use_phnseq=True (the egs/lj recipe) is supported: grapheme input needs nntts.text")
        if phnset_path is None:
            raise ValueError("Please provide phnset_path if want to use phone seq as input")
        self.audiopaths_and_text = load_filepaths_and_text(meta_file)
        self.max_wav_value, self.sampling_rate, self.wav_path = max_wav_value, sampling_rate, wav_path
        # a corpus recorded at another rate (one rate per corpus): the files are yielded untouched, the trainer converts the padded batch
        # on the device (efficient_tts_amd.resample.Resampler) in front of the log-mel front-end
        if source_sampling_rate is not None and (isinstance(source_sampling_rate, bool) or not isinstance(source_sampling_rate, int)
                                                 or source_sampling_rate <= 0):
            raise ValueError(f"source_sampling_rate must be a positive integer (Hz), got {source_sampling_rate!r}")
        self.source_sampling_rate = source_sampling_rate
        with open(phnset_path, "r") as f:
            phn_list = [l.strip() for l in f]
        self.phn2idx = dict(zip(phn_list, range(len(phn_list))))
        random.Random(1234).shuffle(self.audiopaths_and_text)            # the reference shuffles once with seed 1234 (:44-45)

    @property
    def phn_map(self):
        return self.phn2idx

    def get_audio(self, filename: str) -> torch.Tensor:
        from scipy.io.wavfile import read
        sr, data = read(os.path.join(self.wav_path, filename.split("/")[-1]))
        if self.source_sampling_rate is not None:
            if sr != self.source_sampling_rate:
                raise ValueError(f"{filename}: sampling rate {sr} != source_sampling_rate {self.source_sampling_rate} "
                                 f"(converted to {self.sampling_rate} on the device)")
        elif sr != self.sampling_rate:
            raise ValueError(f"{filename}: sampling rate {sr} != {self.sampling_rate}")
        if data.dtype != np.int16:
            raise ValueError(f"{filename}: expected 16-bit PCM")
        return torch.from_numpy(np.ascontiguousarray(data))

    def get_text(self, text: str) -> torch.Tensor:
        return torch.LongTensor([self.phn2idx[p] for p in text.split()])

    def __getitem__(self, index: int) -> Tuple[torch.Tensor, torch.Tensor]:
        path, text = self.audiopaths_and_text[index][0], self.audiopaths_and_text[index][1]
        return self.get_text(text), self.get_audio(path)

    def __len__(self) -> int:
        return len(self.audiopaths_and_text)


class SyntheticTextAudio(torch.utils.data.Dataset):
    """Seeded stand-in for a corpus (smoke tests, benchmarks; there is no dataset in this image):
    phoneme ids in [1, num_symbols) and band-limited noise bursts of matching duration."""

    def __init__(self, meta_file: Optional[str] = None, n_items: int = 64, num_symbols: int = 76, min_phones: int = 20,
                 max_phones: int = 60, frames_per_phone: float = 6.0, hop_size: int = 256, seed: int = 1234):
        g = torch.Generator().manual_seed(seed)
        self.items = []
        for _ in range(n_items):
            n = int(torch.randint(min_phones, max_phones + 1, (1,), generator=g))
            text = torch.randint(1, num_symbols, (n,), generator=g)
            L = int(n * frames_per_phone) * hop_size + int(torch.randint(0, hop_size, (1,), generator=g))
            a = torch.randn(L, generator=g)
            a = torch.nn.functional.avg_pool1d(a[None, None], 5, 1, 2)[0, 0] * 0.25
            self.items.append((text, torch.round(a.clamp(-1, 1) * 32767).to(torch.int16)))
        self.phn2idx = {str(i): i for i in range(num_symbols)}

    @property
    def phn_map(self):
        return self.phn2idx

    def __getitem__(self, i):
        return self.items[i]

    def __len__(self):
        return len(self.items)


class TextMelCollate:
    """Pads a list of (text ids, int16 waveform): returns (text_padded [B, T1] long, input_lengths [B] long,
    audio_padded [B, Lmax] int16, audio_lengths [B] long), items sorted by decreasing text length
    (taco2_data.py:107-117).  n_frames_per_step is accepted for YAML compatibility (the recipe uses 1)."""

    def __init__(self, n_frames_per_step: int = 1):
        if n_frames_per_step != 1:
            raise NotImplementedError("n_frames_per_step != 1 is not used by the EFTS-CNN recipe")
        self.n_frames_per_step = n_frames_per_step

    def __call__(self, batch):
        input_lengths, order = torch.sort(torch.LongTensor([len(x[0]) for x in batch]), dim=0, descending=True)
        B = len(batch)
        text_padded = torch.zeros(B, int(input_lengths[0]), dtype=torch.long)
        audio_lengths = torch.zeros(B, dtype=torch.long)
        Lmax = max(int(x[1].shape[0]) for x in batch)
        audio_padded = torch.zeros(B, Lmax, dtype=torch.int16)
        for i, j in enumerate(order.tolist()):
            text, audio = batch[j]
            text_padded[i, :text.shape[0]] = text
            audio_padded[i, :audio.shape[0]] = audio
            audio_lengths[i] = audio.shape[0]
        return text_padded, input_lengths, audio_padded, audio_lengths
