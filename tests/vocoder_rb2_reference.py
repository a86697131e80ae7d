"""A plain reference of the HiFi-GAN generator with ResBlock2 blocks (`resblock: "2"`, the V3 family) for ANY configuration  --  TEST
INFRASTRUCTURE, imported by tests/test_vocoder_rb2_cpu.py and tests/test_vocoder_rb2_gpu.py.  Importing it needs neither a GPU nor the
library.

Written from the operation (nntts/vocoders/hifigan_model.py:71-93 ResBlock2, :95-136 Generator): a ResBlock2 is
    for c in convs:  x = c(leaky_relu(x, 0.1)) + x
over exactly two weight-normed dilated Conv1d (dilation[0], dilation[1], padding (k d - d) / 2).  Everything around the blocks
(conv_pre, the transposed convolutions, the mean, conv_post) is tests/vocoder_reference.py's, which this module extends.

    param_shapes(cfg)  fill(cfg, seed)  Reference(cfg, P, dtype) with res_block(n, x), res_turn(n, t, x), forward(mel, lengths)

CASES are the configurations of tests/test_vocoder_rb2_gpu.py (the table there says what each covers).
"""
import zlib
from typing import Dict

import torch
import torch.nn.functional as F

import vocoder_reference as VR

LRELU_SLOPE = VR.LRELU_SLOPE

V3 = dict(resblock="2", upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8], upsample_initial_channel=256,
          resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]], num_mels=80)
_NARROW = dict(resblock="2", upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=32,
               resblock_kernel_sizes=[3, 11], resblock_dilation_sizes=[[1, 3], [1, 5]], num_mels=20)
# the golden fixture's configuration (tools/gen_golden_hifigan_rb2.py)
GOLDEN = dict(resblock="2", upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=64,
              resblock_kernel_sizes=[3, 7], resblock_dilation_sizes=[[1, 2], [3, 12]], num_mels=80)   # (the reference builds conv_pre for 80 mels only, :101)
GOLDEN_T, GOLDEN_SEED = 7, 11

# name -> configuration, frames per item, padded length T, seed of the weights and of the mel
CASES = {
    "v3-small": dict(cfg=V3, lengths=[5, 3], T=5, seed=21),
    "narrow": dict(cfg=_NARROW, lengths=[9, 1, 14], T=14, seed=22),
    "limit": dict(cfg=dict(resblock="2", upsample_rates=[4, 4], upsample_kernel_sizes=[8, 8], upsample_initial_channel=64,
                           resblock_kernel_sizes=[9], resblock_dilation_sizes=[[4, 12]], num_mels=20),
                  lengths=[13, 13], T=13, seed=23),
    # one item of 90 frames: 720 rows of 8 channels at the last stage; the k = 11 block's row tile there is 192 - 2 * 25 = 142 rows
    # (5.07 tiles) and the k = 3 block's 192 - 2 * 3 = 186 (3.87 tiles): more than three tiles each, no multiple of either
    "tiles": dict(cfg=_NARROW, lengths=[90], T=90, seed=24),
}


def param_shapes(cfg) -> Dict[str, tuple]:
    """state_dict keys and shapes of the reference Generator for a `resblock: "2"` cfg, in registration order (:100-115)"""
    sh: Dict[str, tuple] = {}

    def wn(prefix, wshape, bias):
        sh[prefix + ".bias"] = (bias,)
        sh[prefix + ".weight_g"] = (wshape[0], 1, 1)
        sh[prefix + ".weight_v"] = wshape

    c0 = int(cfg["upsample_initial_channel"])
    wn("conv_pre", (c0, int(cfg.get("num_mels", 80)), 7), c0)
    for i, k in enumerate(cfg["upsample_kernel_sizes"]):
        wn(f"ups.{i}", (VR.channels(cfg, i - 1), VR.channels(cfg, i), k), VR.channels(cfg, i))
    n = 0
    for i in range(len(cfg["upsample_rates"])):
        ch = VR.channels(cfg, i)
        for k, ds in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]):
            for d in range(2):
                wn(f"resblocks.{n}.convs.{d}", (ch, ch, k), ch)
            n += 1
    wn("conv_post", (1, VR.channels(cfg, len(cfg["upsample_rates"]) - 1), 7), 1)
    return sh


def fill(cfg, seed: int = 0) -> Dict[str, torch.Tensor]:
    """deterministic float32 parameters by the rule of tests/vocoder_reference.py:fill (direction ~ N(0, 1), gain from the fan-in,
    small biases), keyed by parameter name and seed"""
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


class Reference(VR.Reference):
    """conv_pre, up, mean, conv_post of tests/vocoder_reference.py; the residual blocks are ResBlock2"""

    def res_turn(self, n: int, t: int, x):
        """x + convs[t](leaky(x)) of resblocks[n] (ResBlock2.forward :81-88, one turn of its loop)"""
        j = n % len(self.res_kernels)
        k, d = self.res_kernels[j], self.res_dilations[j][t]
        x = x.to(self.dtype)
        xt = F.conv1d(F.leaky_relu(x, LRELU_SLOPE), self.w[f"resblocks.{n}.convs.{t}"], self.b[f"resblocks.{n}.convs.{t}"],
                      padding=(k * d - d) // 2, dilation=d)
        return xt + x

    def res_block(self, n: int, x):
        return self.res_turn(n, 1, self.res_turn(n, 0, x))

    def _forward_dense(self, mel) -> Dict[str, torch.Tensor]:
        st = {"pre": self.conv_pre(mel)}
        x = st["pre"]
        for i in range(len(self.rates)):
            x = st[f"up{i}"] = self.up(i, x)
            finals = []
            for j in range(len(self.res_kernels)):
                finals.append(self.res_block(self.block(i, j), x))
                st[f"r{i}.{j}"] = finals[-1]
            x = st[f"mean{i}"] = self.mean(finals)
        st["out"] = self.conv_post(x)
        return st


def forward(P, mel, lengths=None, cfg=V3, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """every item alone on its unpadded frames, zero-filled past its length (`lengths` None: the dense batch)"""
    return Reference(cfg, P, dtype).forward(mel, lengths)
