"""A plain reference of the HiFi-GAN generator (ResBlock1) for ANY configuration  --  TEST INFRASTRUCTURE, imported by
tests/test_vocoder_reference_cpu.py and tests/test_vocoder_stages_gpu.py.  Plain module: importing it needs neither a GPU nor the library.

Written from the operation (nntts/vocoders/hifigan_model.py:30-58 ResBlock1, :95-136 Generator): torch.nn.functional.conv1d,
conv_transpose1d, leaky_relu and tanh on [B, C, L] tensors, plus the weight-norm fold g * v / ||v|| over dim 0.  Nothing of
efficient_tts_amd/vocoder.py is in it: no 2-tap form of the transposed convolution, no row spaces, no masks, no operand planes.

    fill(cfg, seed)               deterministic state dict with the reference's parameter names (fan-in rule of oracle/hifigan_oracle.py)
    Reference(cfg, P, dtype)      one method per step, each taking THAT step's input (so the device's own intermediate can be fed):
        conv_pre(mel)  up(i, x)  res_pair(n, d_i, r)  mean(list)  conv_post(x)
        forward(mel, lengths)     composes the steps, returns every named stage
    forward(P, mel, lengths, cfg, dtype)    the same as a function

`up` and `conv_post` apply the LeakyReLU of their input first; `activated=True` says the input already went through it (the device
keeps those inputs only as the operand plane of leaky(x)).
`lengths`: every item is run ALONE on its unpadded frames and the result is zero-filled past its length  --  the definition
`HiFiGANGenerator.forward(mel, lengths)` claims.

CASES are the configurations of the stage tests (tests/test_vocoder_stages_gpu.py says what each one covers).
"""
import zlib
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

LRELU_SLOPE = 0.1
POST_SLOPE = 0.01              # F.leaky_relu's default, in front of conv_post (:129)

V1 = dict(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
          resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80)

# name -> configuration, frames per item, padded length T, seed of the weights and of the mel
CASES = {
    "narrow": dict(cfg=dict(resblock="1", upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=64,
                            resblock_kernel_sizes=[3, 7], resblock_dilation_sizes=[[1, 3], [1, 3, 5]], num_mels=80),
                   lengths=[9, 1, 14], T=14, seed=1),
    "v2ish": dict(cfg=dict(resblock="1", upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4], upsample_initial_channel=32,
                           resblock_kernel_sizes=[11], resblock_dilation_sizes=[[1, 5]], num_mels=20),
                  lengths=[6, 11], T=11, seed=2),
    "gap": dict(cfg=dict(resblock="1", upsample_rates=[4, 4], upsample_kernel_sizes=[8, 8], upsample_initial_channel=64,
                         resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80),
                lengths=[12, 12, 5], T=12, seed=3),
    "resident": dict(cfg=dict(resblock="1", upsample_rates=[4, 4, 2], upsample_kernel_sizes=[8, 8, 4], upsample_initial_channel=64,
                              resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80),
                     lengths=[60], T=60, seed=4),
    "v1-small": dict(cfg=V1, lengths=[5, 3], T=5, seed=5),
}


def channels(cfg, i: int) -> int:
    """channels behind upsampling stage i (-1: in front of the first)"""
    return int(cfg["upsample_initial_channel"]) // 2 ** (i + 1)


def param_shapes(cfg) -> Dict[str, tuple]:
    """state_dict keys and shapes of the reference Generator for `cfg`, in registration order (:100-115)"""
    sh: Dict[str, tuple] = {}

    def wn(prefix, wshape, bias):
        sh[prefix + ".bias"] = (bias,)
        sh[prefix + ".weight_g"] = (wshape[0], 1, 1)               # weight_norm, dim 0
        sh[prefix + ".weight_v"] = wshape

    c0 = int(cfg["upsample_initial_channel"])
    wn("conv_pre", (c0, int(cfg.get("num_mels", 80)), 7), c0)
    for i, k in enumerate(cfg["upsample_kernel_sizes"]):
        wn(f"ups.{i}", (channels(cfg, i - 1), channels(cfg, i), k), channels(cfg, i))      # ConvTranspose1d weight [cin][cout][k]
    n = 0
    for i in range(len(cfg["upsample_rates"])):
        ch = channels(cfg, i)
        for k, ds in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]):
            for grp in ("convs1", "convs2"):
                for d in range(len(ds)):
                    wn(f"resblocks.{n}.{grp}.{d}", (ch, ch, k), ch)
            n += 1
    wn("conv_post", (1, channels(cfg, len(cfg["upsample_rates"]) - 1), 7), 1)
    return sh


def fill(cfg, seed: int = 0) -> Dict[str, torch.Tensor]:
    """deterministic float32 parameters: direction v ~ N(0, 1), gain g from the fan-in so that every layer keeps O(1) activations
    (the rule of oracle/hifigan_oracle.py:fill_params: sqrt(||v_slice||^2 / fan_in), fan-in of a transposed convolution = the taps
    that reach one output sample), small biases"""
    shapes = param_shapes(cfg)
    P = {}
    for name, shape in shapes.items():
        g = torch.Generator().manual_seed((zlib.crc32(name.encode()) ^ (seed * 0x9E3779B1)) & 0x7fffffff)
        if name.endswith("weight_v"):
            P[name] = torch.randn(*shape, generator=g)
        elif name.endswith("weight_g"):
            v = shapes[name[:-1] + "v"]
            fan = v[0] * v[2] / cfg["upsample_rates"][int(name.split(".")[1])] if name.startswith("ups") else v[1] * v[2]
            per = (v[1] * v[2]) ** 0.5                                  # ||v|| of one dim-0 slice
            P[name] = (per / fan ** 0.5) * (0.8 + 0.4 * torch.rand(*shape, generator=g))
        else:
            P[name] = 0.1 * torch.randn(*shape, generator=g)
    return P


def mel_input(cfg, B: int, T: int, seed: int) -> torch.Tensor:
    """[B, num_mels, T] float32, padding frames NOT zero (they must not matter)"""
    return torch.randn(B, int(cfg.get("num_mels", 80)), T, generator=torch.Generator().manual_seed(1000 + seed))


class Reference:
    def __init__(self, cfg, P: Dict[str, torch.Tensor], dtype=torch.float64):
        self.cfg, self.dtype = cfg, dtype
        self.rates, self.kernels = list(cfg["upsample_rates"]), list(cfg["upsample_kernel_sizes"])
        self.res_kernels = list(cfg["resblock_kernel_sizes"])
        self.res_dilations = [list(d) for d in cfg["resblock_dilation_sizes"]]
        self.w, self.b = {}, {}
        for name in P:
            if name.endswith(".weight_v"):
                pre = name[:-len(".weight_v")]
                v, g = P[name].to(dtype), P[pre + ".weight_g"].to(dtype)
                self.w[pre] = g * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)
            elif name.endswith(".weight"):                              # weight norm already removed
                self.w[name[:-len(".weight")]] = P[name].to(dtype)
            elif name.endswith(".bias"):
                self.b[name[:-len(".bias")]] = P[name].to(dtype)

    @property
    def hop(self) -> int:
        h = 1
        for u in self.rates:
            h *= u
        return h

    # ---------------------------------------------------------------- the steps ([B, C, L] in, [B, C', L'] out)
    def conv_pre(self, mel):
        return F.conv1d(mel.to(self.dtype), self.w["conv_pre"], self.b["conv_pre"], padding=3)                       # :118

    def up(self, i: int, x, activated: bool = False):
        x = x.to(self.dtype)
        if not activated:
            x = F.leaky_relu(x, LRELU_SLOPE)                                                                        # :120
        u, k = self.rates[i], self.kernels[i]
        return F.conv_transpose1d(x, self.w[f"ups.{i}"], self.b[f"ups.{i}"], stride=u, padding=(k - u) // 2)         # :121

    def block(self, i: int, j: int) -> int:
        """index of residual block j of stage i in `resblocks`"""
        return i * len(self.res_kernels) + j

    def res_pair(self, n: int, d_i: int, r):
        """r + convs2[d_i](leaky(convs1[d_i](leaky(r)))) of resblocks[n] (ResBlock1.forward :45-52, one turn of its loop)"""
        j = n % len(self.res_kernels)
        k, d = self.res_kernels[j], self.res_dilations[j][d_i]
        r = r.to(self.dtype)
        xt = F.leaky_relu(r, LRELU_SLOPE)
        xt = F.conv1d(xt, self.w[f"resblocks.{n}.convs1.{d_i}"], self.b[f"resblocks.{n}.convs1.{d_i}"], padding=(k * d - d) // 2, dilation=d)
        xt = F.leaky_relu(xt, LRELU_SLOPE)
        xt = F.conv1d(xt, self.w[f"resblocks.{n}.convs2.{d_i}"], self.b[f"resblocks.{n}.convs2.{d_i}"], padding=(k - 1) // 2)
        return xt + r

    def mean(self, xs: List[torch.Tensor]):
        s = None
        for x in xs:                                                                                                # :123-127
            s = x.to(self.dtype) if s is None else s + x.to(self.dtype)
        return s / len(xs)                                                                                          # :128

    def conv_post(self, x, activated: bool = False):
        x = x.to(self.dtype)
        if not activated:
            x = F.leaky_relu(x, POST_SLOPE)                                                                         # :129
        return torch.tanh(F.conv1d(x, self.w["conv_post"], self.b["conv_post"], padding=3))                          # :130-131

    # ---------------------------------------------------------------- all of it
    def _forward_dense(self, mel) -> Dict[str, torch.Tensor]:
        st = {"pre": self.conv_pre(mel)}
        x = st["pre"]
        for i in range(len(self.rates)):
            x = st[f"up{i}"] = self.up(i, x)
            finals = []
            for j in range(len(self.res_kernels)):
                r = x
                for d_i in range(len(self.res_dilations[j])):
                    r = st[f"r{i}.{j}.{d_i}"] = self.res_pair(self.block(i, j), d_i, r)
                finals.append(r)
            x = st[f"mean{i}"] = self.mean(finals)
        st["out"] = self.conv_post(x)
        return st

    def forward(self, mel, lengths: Optional[List[int]] = None) -> Dict[str, torch.Tensor]:
        """mel [B, num_mels, T] -> {"pre", "up{i}", "r{i}.{j}.{d}", "mean{i}", "out"}, each [B, C, T * rate of its stage]"""
        if lengths is None:
            return self._forward_dense(mel)
        B, _, T = mel.shape
        out: Dict[str, torch.Tensor] = {}
        for b, n in enumerate(int(v) for v in lengths):
            if n == 0:
                continue
            one = self._forward_dense(mel[b:b + 1, :, :n])
            for name, v in one.items():
                if name not in out:
                    out[name] = torch.zeros(B, v.shape[1], v.shape[2] // n * T, dtype=self.dtype)
                out[name][b, :, :v.shape[2]] = v[0]
        return out


def forward(P, mel, lengths=None, cfg=V1, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    return Reference(cfg, P, dtype).forward(mel, lengths)


def step_refs(cfg, P, mel, lengths) -> Dict[str, tuple]:
    """{stage: (ref64, ref32)}: every step in float64 and in float32 on the SAME float32 input, which is the float64 forward's own
    intermediate rounded to float32  --  what the stage tests do with the device's intermediate, here without a device.  Items alone on
    their unpadded frames, concatenated along time."""
    R64, R32 = Reference(cfg, P, torch.float64), Reference(cfg, P, torch.float32)
    refs: Dict[str, list] = {}

    def both(name, fn, *xs):
        xs = [[v.float() for v in x] if isinstance(x, list) else x.float() for x in xs]
        refs.setdefault(name, []).append((fn(R64, *xs), fn(R32, *xs)))

    for b, n in enumerate(lengths):
        m = mel[b:b + 1, :, :n]
        st = R64._forward_dense(m)
        both("pre", lambda R, x: R.conv_pre(x), m)
        x = st["pre"]
        for i in range(len(R64.rates)):
            both(f"up{i}", lambda R, x: R.up(i, x), x)
            for j in range(len(R64.res_kernels)):
                r = st[f"up{i}"]
                for d_i in range(len(R64.res_dilations[j])):
                    both(f"r{i}.{j}.{d_i}", lambda R, r: R.res_pair(R.block(i, j), d_i, r), r)
                    r = st[f"r{i}.{j}.{d_i}"]
            both(f"mean{i}", lambda R, xs: R.mean(xs), [st[f"r{i}.{j}.{len(R64.res_dilations[j]) - 1}"] for j in range(len(R64.res_kernels))])
            x = st[f"mean{i}"]
        both("out", lambda R, x: R.conv_post(x), x)
    return {k: (torch.cat([a for a, _ in v], 2), torch.cat([c for _, c in v], 2)) for k, v in refs.items()}
