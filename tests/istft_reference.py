"""A plain reference of the iSTFTNet head (Kaneko et al., ICASSP 2022) on the HiFi-GAN trunk  --  TEST INFRASTRUCTURE, imported by
tests/test_istft_reference_cpu.py, tests/test_istft_head_gpu.py and tests/test_istft_cli.py.  Importing it needs neither a GPU nor the
library.

The trunk (conv_pre, the transposed convolutions, the residual blocks, the mean) is tests/vocoder_reference.py's (`resblock: "1"`) or
tests/vocoder_rb2_reference.py's (`resblock: "2"`), which this module extends by import.  The head is written from the formula of
include/efts_abi.h ("The head of an iSTFTNet generator"), in the dtype it is given, with an explicit loop over the frames for the
overlap-add and no torch.istft:

    window(N, dtype)                    periodic Hann, 0.5 - 0.5 cos(2 pi n / N), built in float64
    head(z, N, h, dtype)                z [L + 1, N + 2] (frames x channels) -> the h * L samples
    param_shapes(cfg)  fill(cfg, seed)  the trunk's parameters with the N + 2-channel conv_post
    reference(cfg, P, dtype)            the trunk's Reference with conv_post_z / conv_post_istft; conv_post is the iSTFT head, so
                                        forward(mel, lengths) runs the whole generator, every item alone
    ISTFT_CASES                         the configurations of tests/test_istft_head_gpu.py
"""
import math
import zlib
from typing import Dict

import torch
import torch.nn.functional as F

import vocoder_rb2_reference as RB2
import vocoder_reference as VR

POST_SLOPE = VR.POST_SLOPE

# name -> configuration, frames per item, padded length T, seed of the weights and of the mel
ISTFT_CASES = {
    "c4c4i": dict(cfg=dict(resblock="1", upsample_rates=[4, 4], upsample_kernel_sizes=[8, 8], upsample_initial_channel=64,
                           resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80,
                           gen_istft_n_fft=16, gen_istft_hop_size=4),
                  lengths=[12, 12, 5], T=12, seed=31),
    "rb2-n8": dict(cfg=dict(resblock="2", upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=32,
                            resblock_kernel_sizes=[3, 7], resblock_dilation_sizes=[[1, 3], [1, 3]], num_mels=20,
                            gen_istft_n_fft=8, gen_istft_hop_size=2),
                   lengths=[6, 11, 1], T=11, seed=32),
}


def window(N: int, dtype=torch.float64) -> torch.Tensor:
    n = torch.arange(N, dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(2.0 * math.pi * n / N)).to(dtype)


def frames(z: torch.Tensor, N: int, dtype=torch.float64) -> torch.Tensor:
    """z [F, N + 2] -> y [F, N]: spectrum and inverse real DFT of every frame, from the formula"""
    z = z.to(dtype)
    K = N // 2 + 1
    mag, ph = torch.exp(z[:, :K]), torch.sin(z[:, K:])
    re, im = mag * torch.cos(ph), mag * torch.sin(ph)
    n = torch.arange(N, dtype=torch.float64)
    y = re[:, :1] + ((-1.0) ** n).to(dtype)[None, :] * re[:, N // 2:N // 2 + 1]
    acc = torch.zeros(z.shape[0], N, dtype=dtype)
    for k in range(1, N // 2):
        ang = 2.0 * math.pi * ((k * n) % N) / N
        acc = acc + re[:, k:k + 1] * torch.cos(ang).to(dtype)[None, :] - im[:, k:k + 1] * torch.sin(ang).to(dtype)[None, :]
    return (y + 2.0 * acc) / N


def head(z: torch.Tensor, N: int, h: int, dtype=torch.float64) -> torch.Tensor:
    """z [L + 1, N + 2] -> out [h * L]: windowed frames added at hop h in ascending frame order, divided by the window envelope
    summed in the same order, the first N / 2 samples dropped (center=True)"""
    nf = z.shape[0]
    L = nf - 1
    if L <= 0:
        return torch.zeros(0, dtype=dtype)
    w = window(N, dtype)
    y = frames(z, N, dtype)
    num = torch.zeros(h * L + N, dtype=dtype)
    den = torch.zeros(h * L + N, dtype=dtype)
    for f in range(nf):
        num[h * f:h * f + N] += w * y[f]
        den[h * f:h * f + N] += w * w
    lo = N // 2
    return num[lo:lo + h * L] / den[lo:lo + h * L]


def istft_params(cfg):
    return int(cfg["gen_istft_n_fft"]), int(cfg["gen_istft_hop_size"])


def _base(cfg):
    return RB2 if str(cfg.get("resblock", "1")) == "2" else VR


def param_shapes(cfg) -> Dict[str, tuple]:
    """the HiFi-GAN key set unchanged; conv_post has N + 2 output channels"""
    sh = _base(cfg).param_shapes(cfg)
    N, _ = istft_params(cfg)
    c_last = VR.channels(cfg, len(cfg["upsample_rates"]) - 1)
    sh["conv_post.bias"], sh["conv_post.weight_g"], sh["conv_post.weight_v"] = (N + 2,), (N + 2, 1, 1), (N + 2, c_last, 7)
    return sh


def fill(cfg, seed: int = 0) -> Dict[str, torch.Tensor]:
    """deterministic float32 parameters by the rule of tests/vocoder_reference.py:fill (direction ~ N(0, 1), gain from the fan-in, small
    biases), keyed by parameter name and seed"""
    shapes = param_shapes(cfg)
    P = {}
    for name, shape in shapes.items():
        g = torch.Generator().manual_seed((zlib.crc32(name.encode()) ^ (seed * 0x9E3779B1)) & 0x7fffffff)
        if name.endswith("weight_v"):
            P[name] = torch.randn(*shape, generator=g)
        elif name.endswith("weight_g"):
            v = shapes[name[:-1] + "v"]
            fan = v[0] * v[2] / cfg["upsample_rates"][int(name.split(".")[1])] if name.startswith("ups") else v[1] * v[2]
            P[name] = ((v[1] * v[2]) ** 0.5 / fan ** 0.5) * (0.8 + 0.4 * torch.rand(*shape, generator=g))
        else:
            P[name] = 0.1 * torch.randn(*shape, generator=g)
    return P


mel_input = VR.mel_input


class _Head:
    """conv_post of an iSTFTNet generator: reflection pad (1, 0), the N + 2-channel convolution, the head"""

    def conv_post_z(self, x, activated: bool = False):
        """x [1, C, L] -> z [1, N + 2, L + 1]"""
        x = x.to(self.dtype)
        if not activated:
            x = F.leaky_relu(x, POST_SLOPE)
        x = torch.cat([x[:, :, 1:2], x], 2)                            # a'[0] = a[1], a'[m] = a[m - 1]
        return F.conv1d(x, self.w["conv_post"], self.b["conv_post"], padding=3)

    def head_of(self, z):
        """z [B, N + 2, L + 1] -> [B, 1, h * L]"""
        N, h = istft_params(self.cfg)
        return torch.stack([head(zb.t(), N, h, self.dtype) for zb in z])[:, None]

    def conv_post_istft(self, x, activated: bool = False):
        return self.head_of(self.conv_post_z(x, activated))

    def conv_post(self, x, activated: bool = False):
        return self.conv_post_istft(x, activated)


class Reference1(_Head, VR.Reference):
    pass


class Reference2(_Head, RB2.Reference):
    pass


def reference(cfg, P, dtype=torch.float64):
    return (Reference2 if _base(cfg) is RB2 else Reference1)(cfg, P, dtype)


Reference = reference


def forward(P, mel, lengths, cfg, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """every item alone on its unpadded frames, zero-filled past its length; "out" is [B, 1, T * prod(rates) * h]"""
    return reference(cfg, P, dtype).forward(mel, lengths)
