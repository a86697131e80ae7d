"""A plain reference of the BigVGAN generator (Lee et al., ICLR 2023) for ANY configuration  --  TEST INFRASTRUCTURE, imported by
tests/test_bigvgan_reference_cpu.py and tests/test_snake_aa_gpu.py.  Plain module: importing it needs neither a GPU nor the library.

Written from the operation: torch.nn.functional.conv1d, conv_transpose1d, pad and sin on [B, C, L] tensors plus the weight-norm fold.
Nothing of efficient_tts_amd is in it.  The generator part (param_shapes, fill, Reference, CASES) is what a generator on `efts_snake_aa` will be
tested against; today only the activation is used.

    aa_filter()                      float64 [12], the Kaiser-windowed sinc of UpSample1d / DownSample1d at ratio 2
    activation1d(x, a, inv_b)        Activation1d by the torch-op composition: replicate pad, grouped conv_transpose1d, crop, snake,
                                     replicate pad, grouped strided conv1d; in the dtype of x
    activation1d_direct(x, a, inv_b) the direct double-clamp form of include/efts_abi.h, float64, one channel row at a time
    snake_constants(alpha, beta, logscale)   a and inv_b as the host makes them: float64 from the fp32 parameters, rounded once
    param_shapes(cfg) / fill(cfg, seed)      the upstream key set / a deterministic state dict with it
    Reference(cfg, P, dtype)         one method per step, each taking THAT step's input: conv_pre, up, act, conv, mean, conv_post; forward

CASES are small configurations for stage-by-stage tests of a generator.
"""
import math
import zlib
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

TAPS = 12
PINNED = (0.0020289664498962423, 0.00938946394406788, -0.02554346406529466, -0.05765737547536495, 0.12857260908132875, 0.4432098000653667)


def aa_filter() -> torch.Tensor:
    """kaiser_sinc_filter1d(cutoff 0.25, half_width 0.3, 12) of the upstream project, float64"""
    cutoff, half_width = 0.25, 0.3
    A = 2.285 * (TAPS // 2 - 1) * math.pi * (4 * half_width) + 7.95
    beta = 0.1102 * (A - 8.7)
    w = torch.kaiser_window(TAPS, beta=beta, periodic=False, dtype=torch.float64)
    t = torch.arange(TAPS, dtype=torch.float64) - (TAPS - 1) / 2            # k - 5.5
    f = 2 * cutoff * w * torch.sinc(2 * cutoff * t)
    return f / f.sum()


def activation1d(x: torch.Tensor, a: torch.Tensor, inv_b: torch.Tensor) -> torch.Tensor:
    """x [B, C, L] -> [B, C, L] in x.dtype; a, inv_b [C].  The filter is the float64 one rounded once to float32, then cast to x.dtype
    (the numbers the kernel has compiled in)."""
    dt, C = x.dtype, x.shape[1]
    f = aa_filter().float().to(dt).view(1, 1, TAPS).expand(C, -1, -1)
    u = F.pad(x, (5, 5), mode="replicate")                                   # UpSample1d: pad = 12 / 2 - 1
    u = 2 * F.conv_transpose1d(u, f, stride=2, groups=C)[..., 15:-15]        # pad_left = pad_right = 5 * 2 + (12 - 2) / 2
    v = u + inv_b.to(dt).view(1, C, 1) * torch.sin(u * a.to(dt).view(1, C, 1)) ** 2
    v = F.pad(v, (5, 6), mode="replicate")                                   # LowPassFilter1d, even kernel: 12 / 2 - 1 and 12 / 2
    return F.conv1d(v, f, stride=2, groups=C)


def activation1d_direct(x: torch.Tensor, a: torch.Tensor, inv_b: torch.Tensor) -> torch.Tensor:
    """the definition of include/efts_abi.h in float64: x [C, L] -> [C, L]"""
    f = aa_filter().float().double()
    x, a, inv_b = x.double(), a.double().view(-1, 1), inv_b.double().view(-1, 1)
    C, L = x.shape

    def X(i):
        return x[:, min(max(i, 0), L - 1)]

    def v(m):
        m = min(max(m, 0), 2 * L - 1)
        j = m >> 1
        u = torch.zeros(C, dtype=torch.float64)
        for i in range(6):
            u = u + (f[2 * i + 1] * X(j + 2 - i) if m % 2 == 0 else f[2 * i] * X(j + 3 - i))
        u = 2 * u
        return u + inv_b[:, 0] * torch.sin(a[:, 0] * u) ** 2

    vs = {m: v(m) for m in range(-5, 2 * L + 6)}
    y = torch.zeros(C, L, dtype=torch.float64)
    for t in range(L):
        for k in range(TAPS):
            y[:, t] = y[:, t] + f[k] * vs[2 * t + k - 5]
    return y


def snake_constants(alpha: torch.Tensor, beta: Optional[torch.Tensor], logscale: bool):
    """(a, inv_b) float32: a = exp(alpha) or alpha; inv_b = 1 / (a + 1e-9) (Snake) or 1 / (b + 1e-9), b from beta the same way"""
    def lin(p):
        p = p.detach().double()
        return p.exp() if logscale else p
    a = lin(alpha)
    b = a if beta is None else lin(beta)
    return a.float(), (1.0 / (b + 1e-9)).float()


BASE = dict(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
            resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80,
            activation="snakebeta", snake_logscale=True)

# name -> configuration, frames per item, padded length T, seed of the weights and of the mel, the precisions the case runs in
CASES = {
    "amp-narrow": dict(cfg=dict(resblock="1", upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=32,
                                resblock_kernel_sizes=[3, 7], resblock_dilation_sizes=[[1, 3], [1, 3, 5]], num_mels=80,
                                activation="snakebeta", snake_logscale=True),
                       lengths=[9, 1, 14], T=14, seed=11, precisions=("fp32", "bf16x3", "bf16")),
    "amp-snake": dict(cfg=dict(resblock="1", upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4], upsample_initial_channel=32,
                               resblock_kernel_sizes=[11], resblock_dilation_sizes=[[1, 5]], num_mels=20, activation="snake"),
                      lengths=[6, 11], T=11, seed=12, precisions=("fp32", "bf16x3", "bf16")),
    "amp2": dict(cfg=dict(resblock="2", upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=32,
                          resblock_kernel_sizes=[3, 5], resblock_dilation_sizes=[[1, 2], [2, 6]], num_mels=80,
                          activation="snakebeta", snake_logscale=True),
                 lengths=[7, 3], T=7, seed=13, precisions=("fp32", "bf16x3", "bf16")),
    "amp-wide": dict(cfg=dict(resblock="1", upsample_rates=[8, 8], upsample_kernel_sizes=[16, 16], upsample_initial_channel=512,
                              resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80,
                              activation="snakebeta", snake_logscale=True),
                     lengths=[3, 2], T=3, seed=14, precisions=("fp32", "bf16x3")),
}


def channels(cfg, i: int) -> int:
    """channels behind upsampling stage i (-1: in front of the first)"""
    return int(cfg["upsample_initial_channel"]) // 2 ** (i + 1)


def act_count(cfg, j: int) -> int:
    """activations of a residual block of kernel j"""
    return len(cfg["resblock_dilation_sizes"][j]) * (2 if str(cfg.get("resblock", "1")) == "1" else 1)


def param_shapes(cfg) -> Dict[str, tuple]:
    """state_dict keys and shapes of the upstream BigVGAN generator for `cfg`"""
    sh: Dict[str, tuple] = {}
    beta = cfg["activation"] == "snakebeta"

    def wn(prefix, wshape, bias=True):
        if bias:
            sh[prefix + ".bias"] = (wshape[0] if not prefix.startswith("ups") else wshape[1],)
        sh[prefix + ".weight_g"] = (wshape[0], 1, 1)
        sh[prefix + ".weight_v"] = wshape

    def act(prefix, c):
        sh[prefix + ".act.alpha"] = (c,)
        if beta:
            sh[prefix + ".act.beta"] = (c,)
        sh[prefix + ".upsample.filter"] = (1, 1, TAPS)
        sh[prefix + ".downsample.lowpass.filter"] = (1, 1, TAPS)

    c0 = int(cfg["upsample_initial_channel"])
    wn("conv_pre", (c0, int(cfg.get("num_mels", 80)), 7))
    for i, k in enumerate(cfg["upsample_kernel_sizes"]):
        wn(f"ups.{i}.0", (channels(cfg, i - 1), channels(cfg, i), k))
    n, one = 0, str(cfg.get("resblock", "1")) == "1"
    for i in range(len(cfg["upsample_rates"])):
        ch = channels(cfg, i)
        for j, (k, ds) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            for grp in (("convs1", "convs2") if one else ("convs",)):
                for d in range(len(ds)):
                    wn(f"resblocks.{n}.{grp}.{d}", (ch, ch, k))
            for l in range(act_count(cfg, j)):
                act(f"resblocks.{n}.activations.{l}", ch)
            n += 1
    c_last = channels(cfg, len(cfg["upsample_rates"]) - 1)
    act("activation_post", c_last)
    wn("conv_post", (1, c_last, 7), bias=bool(cfg.get("use_bias_at_final", True)))
    return sh


def fill(cfg, seed: int = 0) -> Dict[str, torch.Tensor]:
    """deterministic float32 parameters: the rule of tests/vocoder_reference.py for the convolutions; alpha and beta with a and b around 1
    (logarithms under snake_logscale); the filter buffers hold the constant"""
    shapes, log = param_shapes(cfg), bool(cfg.get("snake_logscale", False))
    P = {}
    for name, shape in shapes.items():
        g = torch.Generator().manual_seed((zlib.crc32(name.encode()) ^ (seed * 0x9E3779B1)) & 0x7fffffff)
        if name.endswith("weight_v"):
            P[name] = torch.randn(*shape, generator=g)
        elif name.endswith("weight_g"):
            v = shapes[name[:-1] + "v"]
            fan = v[0] * v[2] / cfg["upsample_rates"][int(name.split(".")[1])] if name.startswith("ups") else v[1] * v[2]
            P[name] = ((v[1] * v[2]) ** 0.5 / fan ** 0.5) * (0.8 + 0.4 * torch.rand(*shape, generator=g))
        elif name.endswith("filter"):
            P[name] = aa_filter().float().view(1, 1, TAPS)
        elif name.endswith("alpha") or name.endswith("beta"):
            e = 0.4 * torch.randn(*shape, generator=g)
            P[name] = e if log else e.exp()
        else:
            P[name] = 0.1 * torch.randn(*shape, generator=g)
    return P


def mel_input(cfg, B: int, T: int, seed: int) -> torch.Tensor:
    """[B, num_mels, T] float32, padding frames NOT zero (they must not matter)"""
    return torch.randn(B, int(cfg.get("num_mels", 80)), T, generator=torch.Generator().manual_seed(2000 + seed))


class Reference:
    def __init__(self, cfg, P: Dict[str, torch.Tensor], dtype=torch.float64):
        self.cfg, self.dtype, self.P = cfg, dtype, P
        self.rates, self.kernels = list(cfg["upsample_rates"]), list(cfg["upsample_kernel_sizes"])
        self.res_kernels = list(cfg["resblock_kernel_sizes"])
        self.res_dilations = [list(d) for d in cfg["resblock_dilation_sizes"]]
        self.one = str(cfg.get("resblock", "1")) == "1"
        self.log = bool(cfg.get("snake_logscale", False))
        self.final_tanh = bool(cfg.get("use_tanh_at_final", True))
        self.w, self.b = {}, {}
        for name in P:
            if name.endswith(".weight_v"):
                pre = name[:-len(".weight_v")]
                v, g = P[name].to(dtype), P[pre + ".weight_g"].to(dtype)
                self.w[pre] = g * v / v.flatten(1).norm(dim=1).view(-1, 1, 1)
            elif name.endswith(".bias"):
                self.b[name[:-len(".bias")]] = P[name].to(dtype)

    # ---------------------------------------------------------------- the steps ([B, C, L] in, [B, C', L'] out)
    def conv_pre(self, mel):
        return F.conv1d(mel.to(self.dtype), self.w["conv_pre"], self.b["conv_pre"], padding=3)

    def up(self, i: int, x):
        u, k = self.rates[i], self.kernels[i]
        return F.conv_transpose1d(x.to(self.dtype), self.w[f"ups.{i}.0"], self.b[f"ups.{i}.0"], stride=u, padding=(k - u) // 2)

    def act(self, prefix: str, x):
        """Activation1d with the parameters under `prefix` ("resblocks.{n}.activations.{l}" or "activation_post")"""
        a, inv_b = snake_constants(self.P[prefix + ".act.alpha"], self.P.get(prefix + ".act.beta"), self.log)
        return activation1d(x.to(self.dtype), a, inv_b)

    def conv(self, name: str, x, k: int, d: int, resid=None):
        y = F.conv1d(x.to(self.dtype), self.w[name], self.b[name], padding=(k * d - d) // 2, dilation=d)
        return y if resid is None else y + resid.to(self.dtype)

    def block(self, i: int, j: int) -> int:
        return i * len(self.res_kernels) + j

    def mean(self, xs: List[torch.Tensor]):
        s = None
        for x in xs:
            s = x.to(self.dtype) if s is None else s + x.to(self.dtype)
        return s / len(xs)

    def conv_post(self, x):
        """conv_post and tanh (or the clamp) on the plane activation_post wrote"""
        y = F.conv1d(x.to(self.dtype), self.w["conv_post"], self.b.get("conv_post"), padding=3)
        return torch.tanh(y) if self.final_tanh else y.clamp(-1.0, 1.0)

    # ---------------------------------------------------------------- all of it
    def _forward_dense(self, mel) -> torch.Tensor:
        x = self.conv_pre(mel)
        for i in range(len(self.rates)):
            x = self.up(i, x)
            finals = []
            for j, (k, ds) in enumerate(zip(self.res_kernels, self.res_dilations)):
                n, r = self.block(i, j), x
                for d_i, d in enumerate(ds):
                    if self.one:
                        xt = self.conv(f"resblocks.{n}.convs1.{d_i}", self.act(f"resblocks.{n}.activations.{2 * d_i}", r), k, d)
                        r = self.conv(f"resblocks.{n}.convs2.{d_i}", self.act(f"resblocks.{n}.activations.{2 * d_i + 1}", xt), k, 1, resid=r)
                    else:
                        r = self.conv(f"resblocks.{n}.convs.{d_i}", self.act(f"resblocks.{n}.activations.{d_i}", r), k, d, resid=r)
                finals.append(r)
            x = self.mean(finals)
        return self.conv_post(self.act("activation_post", x))

    def forward(self, mel, lengths: Optional[List[int]] = None) -> torch.Tensor:
        """mel [B, num_mels, T] -> audio [B, 1, T * hop]; with lengths every item runs ALONE on its unpadded frames, zeros past its length"""
        if lengths is None:
            return self._forward_dense(mel)
        B, _, T = mel.shape
        hop = math.prod(self.rates)
        out = torch.zeros(B, 1, T * hop, dtype=self.dtype)
        for b, n in enumerate(int(v) for v in lengths):
            if n:
                out[b, :, :n * hop] = self._forward_dense(mel[b:b + 1, :, :n])[0]
        return out
