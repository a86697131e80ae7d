"""On-device Griffin-Lim vocoder: log-mel -> waveform by phase reconstruction, the inverse of `frontend.LogMelFrontend`.

Needs no weights and is deterministic, so a checkout can turn the acoustic model's mel-spectrograms into audio one can listen to
(intelligible, not HiFi-GAN quality) and the tests get an audio-domain check of a mel that depends on no checkpoint.
Algorithm: Griffin & Lim 1984 with the momentum term of Perraudin, Balazs & Sondergaard 2013, for the reference's analysis
configuration (n_fft 1024, hop 256, window 1024, periodic Hann, Slaney mel bins; meldataset.py:49-82).

Conventions (analysis and synthesis are inverses of each other): the front-end reflect-pads 384 samples per side and frames
without centring, so frame t starts at padded sample 256 t and T frames describe 256 T samples.  The vocoder works on the padded
signal y_pad of 256 T + 768 samples and returns y_pad[384 : 384 + 256 T].

  1. M = max(pinv(FB) @ exp(logmel), 1e-5): the pseudo-inverse of the Slaney filterbank (float64, numpy, once on the host) as a
     packed weight of the project's MFMA contraction (`ops.gemm`, operand format bf16x3 or fp32);
  2. X_0 = M e^(i phi), phi = 0 (`init="zero"`) or hashed uniform phases (`init="random"`, `seed`); Y_prev = 0;
  3. synthesis: y = overlap-add(hann * irfft(X)) / (sum of hann^2 over the frames that cover the sample, floor 1e-8);
  4. analysis + projection: Y = rfft(hann * frames(y)); C = Y + a (Y - Y_prev); X = M C / max(|C|, 1e-8); Y_prev = Y;
  5. `n_iter` times 3 + 4, then one last synthesis.  (Y_prev = 0 makes the first projection the plain one: C = (1 + a) Y.)

Kernels: csrc/efts_griffinlim.hip -- two launches per iteration (`efts_gl_synthesis`, `efts_gl_analysis`; the time signal never
exists inside the loop: the analysis gathers every sample from the up to four windowed frames that cover it, in a fixed order), the
whole call replayed as one hipGraph per (B, T).  No CPU path: the HIP library is required.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import lib as L
from . import ops as O
from .audio_args import Cache
from .frontend import slaney_mel_filterbank
from .graphs import GraphCache
from .ops import F32Rows, PackedWeight, Plane, Rows

MAG_FLOOR = 1e-5
_SPLITS = {"bf16x3": L.SPLIT_BF16X3, "fp32": L.SPLIT_FP32}


def mel_pseudo_inverse(sampling_rate: int, n_fft: int, num_mels: int, fmin: float, fmax: float) -> np.ndarray:
    """pinv(FB) [n_fft / 2 + 1, num_mels] in float64 (FB: frontend.slaney_mel_filterbank)"""
    fb = slaney_mel_filterbank(sampling_rate, n_fft, num_mels, fmin, fmax).astype(np.float64)
    return np.linalg.pinv(fb)


class GriffinLimVocoder(torch.nn.Module):
    """audio = GriffinLimVocoder(device)(mel [B, 80, T], lengths=None) -> [B, 1, 256 T]: the call signature of
    `vocoder.HiFiGANGenerator.forward`.  `lengths` (frames per item, optional): every item is synthesised exactly as if it had
    been passed alone without its padding; samples past lengths[b] * 256 are 0."""

    def __init__(self, device=None, n_iter: int = 32, momentum: float = 0.99, init: str = "zero", seed: int = 0, precision: str = "bf16x3",
                 sampling_rate: int = 22050, n_fft: int = 1024, hop_size: int = 256, win_size: int = 1024, num_mels: int = 80,
                 fmin: float = 0.0, fmax: float = 8000.0, graphs: bool = True):
        super().__init__()
        if win_size != n_fft:
            raise ValueError("win_size must equal n_fft (the reference's configuration)")
        if n_fft != 1024 or hop_size != 256 or not 0 < num_mels <= 80:
            raise ValueError("the Griffin-Lim vocoder is built for n_fft 1024, hop 256, at most 80 mel bins (what LogMelFrontend(radix=0) covers)")
        if int(n_iter) != n_iter or n_iter < 0:
            raise ValueError("n_iter must be a non-negative integer")
        if not 0.0 <= momentum < 1.0:
            raise ValueError("momentum must lie in [0, 1)")
        if init not in ("zero", "random"):
            raise ValueError("init must be 'zero' or 'random'")
        if precision not in _SPLITS:
            raise ValueError("precision must be 'bf16x3' or 'fp32'")
        self.dev = None if device is None else torch.device(device)
        self.n_iter, self.momentum, self.init, self.seed = int(n_iter), float(momentum), init, int(seed) & 0xFFFFFFFF
        self.precision, self.split = precision, _SPLITS[precision]
        self.n_fft, self.hop, self.num_mels, self.n_bins = n_fft, hop_size, num_mels, n_fft // 2 + 1
        self.pad = (n_fft - hop_size) // 2
        self.graphs = graphs
        self._pinv_host = torch.from_numpy(mel_pseudo_inverse(sampling_rate, n_fft, num_mels, fmin, fmax).astype(np.float32)).contiguous()
        self._state = {}                 # device -> (packed pinv, window)
        self._ws = Cache(capacity=5)     # (device, B, T) -> buffers
        self._graph_cache = GraphCache(capacity=8)

    # ------------------------------------------------------------------ device state
    def _device_state(self, dev):
        if dev not in self._state:
            with O.stream_scope():
                pinv = PackedWeight(self.n_bins, self.num_mels, 1, self.split, dev)
                pinv.pack(self._pinv_host.to(dev).contiguous())
            window = torch.hann_window(self.n_fft, dtype=torch.float32).to(dev)               # periodic hann, meldataset.py:67
            self._state[dev] = (pinv, window)
        return self._state[dev]

    def _workspace_for(self, B: int, T: int, dev) -> dict:
        def make():
            rs = Rows(B, T)
            return dict(
                rs=rs, mel=Plane.for_rows(rs, self.num_mels, self.split, dev), lin=F32Rows(rs, O.roundup(self.n_bins, 4), dev),
                spec=torch.zeros(B, T, self.n_bins, 2, dtype=torch.float32, device=dev),
                prev=torch.zeros(B, T, self.n_bins, 2, dtype=torch.float32, device=dev),
                wframes=torch.zeros(B, T, self.n_fft, dtype=torch.float32, device=dev))
        return self._ws.get((dev, B, T), make)

    def _check_input(self, x: torch.Tensor) -> None:
        if x.dim() != 3 or x.shape[1] != self.num_mels:
            raise ValueError(f"expected mel [B, {self.num_mels}, T]")
        if not x.is_cuda:
            raise RuntimeError("GriffinLimVocoder runs on an MI355X device only (no CPU path)")
        if x.shape[0] < 1 or x.shape[2] < 1:
            raise ValueError("empty batch or no frames")
        L.load()
        L.require_device()

    # ------------------------------------------------------------------ step 1
    def _magnitude(self, mel: torch.Tensor, ws: dict, pinv: PackedWeight) -> torch.Tensor:
        rs, plane, lin = ws["rs"], ws["mel"], ws["lin"]
        power = torch.exp(mel.float()).transpose(1, 2).contiguous()                       # [B, T, num_mels]: what the filterbank produced before the log
        O.pack_rows(power, None, plane, rs)
        # one tiling for every row count: an item's magnitudes must not depend on the batch it stands in
        O.gemm(a=plane, b_ptr=pinv.ptr, ldb=pinv.ld, m=rs.rows, n=self.n_bins, out_f32_ptr=lin.ptr, ldo=lin.c, tiling=L.TILING_GENERIC)
        return lin.view()[:, :, :self.n_bins].clamp_min(MAG_FLOOR).contiguous()

    @torch.no_grad()
    def magnitude(self, mel: torch.Tensor) -> torch.Tensor:
        """step 1 alone: log-mel [B, num_mels, T] -> linear magnitudes M [B, T, 513]"""
        self._check_input(mel)
        pinv, _ = self._device_state(mel.device)
        with O.stream_scope():
            return self._magnitude(mel, self._workspace_for(mel.shape[0], mel.shape[2], mel.device), pinv)

    # ------------------------------------------------------------------ forward
    def _run(self, mel: torch.Tensor, lens: torch.Tensor, ws: dict, pinv: PackedWeight, window: torch.Tensor) -> torch.Tensor:
        B, _, T = mel.shape
        lib, st = L.load(), O._stream()
        mag = self._magnitude(mel, ws, pinv)
        spec, prev, wf = ws["spec"], ws["prev"], ws["wframes"]
        audio = torch.empty(B, 1, T * self.hop, dtype=torch.float32, device=mel.device)
        L.check(lib.efts_gl_init(mag.data_ptr(), spec.data_ptr(), prev.data_ptr(), B, T, int(self.init == "random"), self.seed, st), "efts_gl_init")
        for _ in range(self.n_iter):
            L.check(lib.efts_gl_synthesis(spec.data_ptr(), lens.data_ptr(), window.data_ptr(), wf.data_ptr(), B, T, self.n_fft, self.hop, st),
                    "efts_gl_synthesis")
            L.check(lib.efts_gl_analysis(wf.data_ptr(), None, 0, lens.data_ptr(), window.data_ptr(), mag.data_ptr(), prev.data_ptr(), spec.data_ptr(),
                                         self.momentum, B, T, self.n_fft, self.hop, st), "efts_gl_analysis")
        L.check(lib.efts_gl_synthesis(spec.data_ptr(), lens.data_ptr(), window.data_ptr(), wf.data_ptr(), B, T, self.n_fft, self.hop, st),
                "efts_gl_synthesis")
        L.check(lib.efts_gl_overlap_add(wf.data_ptr(), lens.data_ptr(), window.data_ptr(), audio.data_ptr(), T * self.hop, self.pad, T * self.hop,
                                        B, T, self.n_fft, self.hop, st), "efts_gl_overlap_add")
        return audio

    @torch.no_grad()
    def forward(self, x: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._check_input(x)
        dev = x.device
        B, _, T = x.shape
        pinv, window = self._device_state(dev)
        if lengths is None:
            lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        else:
            lens = lengths.to(device=dev, dtype=torch.int32).clamp(0, T)
        ws = self._workspace_for(B, T, dev)

        def body(mel, lens_i32):
            with O.stream_scope():
                return (self._run(mel, lens_i32, ws, pinv, window),)

        mel = x.float().contiguous()
        if not self.graphs or torch.cuda.is_current_stream_capturing():
            return body(mel, lens)[0]
        # the graph is valid while the buffers its launches point at live (this workspace, the packed pseudo-inverse) and for the
        # loop it was captured with
        tag = (id(ws), pinv.ptr, self.n_iter, self.momentum, self.init, self.seed)
        return self._graph_cache.run(("gl", dev.index, B, T), tag, (mel, lens), body, keepalive=(ws, pinv, window))[0]
