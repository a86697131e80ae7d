"""HiFi-GAN generators (ResBlock1: V1 / V2; ResBlock2: V3) and iSTFTNet generators (the same trunk under an inverse-STFT head: C8C8I, C8C8C2I)
on the MI355X contraction kernels.

Drop-in for `nntts.vocoders.hifigan_model.Generator` (nntts/vocoders/hifigan_model.py:95-150): same constructor argument (the config object / dict of
a HiFi-GAN config.json), same parameter names and shapes (`state_dict` of the reference loads unchanged, weight_g / weight_v pairs),
`forward(mel [B, num_mels, T]) -> audio [B, 1, T * hop]` (hop = prod(upsample_rates), times N / 4 under an iSTFT head), `remove_weight_norm()`.  Inference only; there is no CPU path.

A forward is a short driver (`_run`) over stages; `_Pass` is what every stage reads, a namedtuple what one hands to the next:
  * `_stage_pre`: the mel as an operand plane, its row mask, conv_pre.  Every Conv1d is one `efts_gemm` launch on channel-last rows (one row per
    sample; a tap offset is a row offset into the LDS window).  Every consumer of a convolution's result applies LeakyReLU first, so the PRODUCER
    writes the operand plane of leaky(x) (`plane_act`) and no activation pass exists;
  * `_stage_upsample`: ConvTranspose1d(stride u, kernel 2u, padding u/2) = a 2-tap convolution with u * cout output columns, y[n] = x[q] w[r] +
    x[q-1] w[r+u] with n + u/2 = q u + r; the [T+1][u*cout] result IS the [u(T+1)][cout] row space of the stage behind an offset of u/2 rows;
  * `_stage_residual`: the residual blocks of the stage are independent chains, the longest kernel issued first, each on a stream of its own but
    the last.  WHAT a chain launches belongs to its block class alone: `_ResBlock1` / `_ResBlock2` say what they refuse, which convolutions they
    pack, which buffers a chain needs and which launches run it.  The generator names a kind once, where it picks the class (`_BLOCKS`);
  * `_stage_mean`: the multi-receptive-field mean and the LeakyReLU of the next layer's input, `efts_mean_act_rows`;
  * `_stage_post`: the head, the only code that knows it.  `_TanhHead` (HiFi-GAN): conv_post with the kernel's tanh epilogue and the copy into the
    audio.  `_IstftHead` (config keys `gen_istft_n_fft` = N, `gen_istft_hop_size` = N / 4; Kaneko et al., ICASSP 2022): the reflected row in front
    of every item, conv_post as an `efts_gemm` launch with N + 2 fp32 columns, and `efts_istft_head` (csrc/efts_istft_head.hip), which writes the
    audio itself: `hop` = prod(upsample_rates) * N / 4 samples per mel frame.
Batches: the B utterances share one row space per stage, item b at rows b * P .. b * P + T_b * up with a pitch of P = (T + gap) * up rows.  `gap`
spare mel frames (`gap_frames`) come from the configuration: at the first upsampled stage they are gap * upsample_rates[0] zero rows, no fewer than
the largest halo of a residual convolution, max (k - 1) / 2 * d; never fewer than 4 frames, which cover conv_pre (3 rows at mel rate) and the extra
input row of the transposed convolutions.  V1: max(4, ceil(25 / 8)) = 4 frames, 32 rows against a halo of (11 - 1) / 2 * 5 = 25.  Every launch
carries the row mask of its stage, so rows past an item's length stay zero exactly as the zero padding of a single-utterance run does: `forward(mel,
lengths)` equals B separate calls on the unpadded items.  What the launches cannot compute is refused in the constructor (`_refusal`), never later.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
from collections import namedtuple
from typing import Dict, List, Optional

import torch
import torch.nn as nn
from torch.nn.utils import remove_weight_norm, weight_norm

from . import lib as L
from . import ops as O
from .audio_args import Cache
from .ops import PackedWeight, Plane

LRELU_SLOPE = 0.1
_GUARD = 64            # zero rows in front of every row space: (taps - 1) / 2 * dilation <= 25
_MIN_GAP_FRAMES = 4    # spare mel frames between the items of a batch, at least: conv_pre's halo (3) and the transposed convolutions' extra row
_MAX_RES_KERNELS = 3   # efts_mean_act_rows adds up to three streams
_GEMM_TAPS = (1, 3, 5, 7, 9, 11)       # what efts_gemm takes as `taps`
_GEMM_MAX_SPAN = 64    # efts_gemm: (taps - 1) * dilation rows of window at the most
_RB2_TAPS = (3, 5, 7, 9, 11)           # what efts_resblock2 takes as `k`
_RB2_MAX_C = 128       # efts_resblock2: channels at the most
_RB2_MAX_HALO = _GUARD  # efts_resblock2: (k - 1) / 2 * (d0 + d1) rows at the most
_ISTFT_N = (8, 16, 32)  # efts_istft_head: transform sizes


def _cfg(h, key, default=None):
    return h[key] if isinstance(h, dict) and key in h else getattr(h, key, default)


def gap_frames(upsample_rates, res_kernels, res_dilations) -> int:
    """spare mel frames between the items of a batch: their rows at the first upsampled stage hold the largest halo of a
    residual convolution (the later stages only have more rows per frame)"""
    halo = max((k - 1) // 2 * d for k, ds in zip(res_kernels, res_dilations) for d in ds)
    return max(_MIN_GAP_FRAMES, -(-halo // upsample_rates[0]))


class _Rows:
    """fp32 [rows][c] stream + its operand plane, both with zero guard rows"""

    def __init__(self, rows: int, c: int, split: int, dev, f32: bool = True, plane: bool = True):
        self.rows, self.c = rows, c
        alloc = _GUARD + O.roundup(rows, 128) + 256
        self.f = torch.zeros(alloc, c, dtype=torch.float32, device=dev) if f32 else None
        self.p = Plane(alloc, c, split, dev, guard_lo=_GUARD) if plane else None

    @property
    def fptr(self) -> int:
        return self.f.data_ptr() + _GUARD * self.c * 4


class _Pass:
    """What every stage of one forward reads.  ws: the workspace of the shape (`_Workspace`); pk: `_Conv` by packed name; B, T: the mel
    batch; pitch: rows per item at mel rate; rate: rows per frame at the last stage; lens: int32 frames per item on the device; dev; st: the main
    stream's handle; split: the operand format; fused: `_rb2_fused`, which arm runs a ResBlock2; keep: the dict the stage tests read, or None"""
    __slots__ = ("ws", "pk", "B", "T", "pitch", "rate", "lens", "dev", "st", "split", "fused", "keep")

    def __init__(self, **fields):
        for k, v in fields.items():
            setattr(self, k, v)


_Conv = namedtuple("_Conv", "w bias")                         # one packed convolution: PackedWeight and its fp32 bias, made together
_Stage = namedtuple("_Stage", "up x chains s mask")           # up: fp32 GEMM result; x, s: planes of leaky(x), leaky(mean); chains: `scratch` per block
_Workspace = namedtuple("_Workspace", "pitch mel pre stages mask_mel head")     # head: what the head class's `scratch` made
_Act = namedtuple("_Act", "p rows")                           # handed on by conv_pre and by a stage's mean: the plane the next contraction reads
_Up = namedtuple("_Up", "x_f x_p mask rows c")                # handed on by the upsampling: fp32 pointer and plane of leaky(x), row mask, rows, channels


def _conv(cv: _Conv, a: Plane, rows, taps, dil, *, mask=None, out_f=None, ldo=0, out_p=None, plane_slope=None, resid=None, ldr=0,
          act=L.ACT_NONE, a_ptr=None):
    O.gemm(a=a, a_ptr=a_ptr, b_ptr=cv.w.ptr, ldb=cv.w.ld, b_tap_stride=cv.w.tap_stride, taps=taps, m=rows, n=cv.w.cout, bias=cv.bias, act=act,
           resid_ptr=resid, ldr=ldr, rowmask_ptr=None if mask is None else mask.data_ptr(), out_f32_ptr=out_f, ldo=ldo,
           out_plane=out_p, dilation=dil, plane_act=plane_slope is not None, plane_slope=0.0 if plane_slope is None else plane_slope)


def _weight_normed(channels: int, k: int, dilations) -> nn.ModuleList:
    return nn.ModuleList([weight_norm(nn.Conv1d(channels, channels, k, 1, dilation=d, padding=(k * d - d) // 2)) for d in dilations])


def _bad_dilation(k: int, d: int) -> str:
    return f"residual kernel size {k} with dilation {d}: efts_gemm takes (k - 1) * d <= {_GEMM_MAX_SPAN} rows, d >= 1"


class _ResBlock1(nn.Module):
    """The reference's parameters under its names (hifigan_model.py:30-52) and everything that depends on the kind; never called.  Pre-activation
    pairs x <- x + conv_{k,1}(leaky(conv_{k,d}(leaky(x)))): `xt` between the two convolutions of a pair only ever lives as an operand plane."""

    def __init__(self, channels: int, kernel_size: int, dilation):
        super().__init__()
        self.convs1 = _weight_normed(channels, kernel_size, dilation)
        self.convs2 = _weight_normed(channels, kernel_size, [1 for _ in dilation])
        self.kernel_size, self.dilation = kernel_size, tuple(dilation)

    @staticmethod
    def refusal(k: int, ds, c_max: int) -> Optional[str]:      # why efts_gemm cannot run a block of this geometry (None: it can)
        return next((_bad_dilation(k, d) for d in ds if d < 1 or (k - 1) * d > _GEMM_MAX_SPAN), None)

    def packed(self, n: int):           # (packed name, module) of block n in launch order
        return [(f"rb{n}.c{t}.{d}", m[d]) for d in range(len(self.dilation)) for t, m in ((1, self.convs1), (2, self.convs2))]

    @staticmethod
    def scratch(chains: int, rows: int, c: int, split: int, dev):     # per chain (they run side by side): the ping-pong pair, the plane of leaky(xt)
        t = [_Rows(rows, c, split, dev, f32=False) for _ in range(chains)]
        return [([_Rows(rows, c, split, dev) for _ in range(2)], t_j) for t_j in t]

    def launch(self, ps: _Pass, n: int, up: _Up, scratch, key: str) -> int:
        """block n on the current stream (:45-52): the pointer of the fp32 result; keeps "{key}.{d}" after pair d"""
        (pp, t), k, r_f, r_p = scratch, self.kernel_size, up.x_f, up.x_p
        for d_i, d in enumerate(self.dilation):
            _conv(ps.pk[f"rb{n}.c1.{d_i}"], r_p, up.rows, k, d, mask=up.mask, out_p=t.p, plane_slope=LRELU_SLOPE)       # :47-48 (+ :49)
            nxt = pp[d_i & 1]
            _conv(ps.pk[f"rb{n}.c2.{d_i}"], t.p, up.rows, k, 1, mask=up.mask, out_f=nxt.fptr, ldo=up.c, out_p=nxt.p,
                  plane_slope=LRELU_SLOPE, resid=r_f, ldr=up.c)                                                          # :50-51
            r_f, r_p = nxt.fptr, nxt.p
            if ps.keep is not None:             # (on this chain's stream: the next pair but one writes this buffer again)
                ps.keep[f"{key}.{d_i}"] = nxt.f.clone()
        return r_f


class _ResBlock2(nn.Module):
    """The reference's parameters under its names (hifigan_model.py:71-93) and everything that depends on the kind; never called.  Two turns
    x <- x + conv_{k,d}(leaky(x)), d = dilation[0], dilation[1], run by ONE `efts_resblock2` launch (csrc/efts_resblock2.hip: the intermediate stays
    in LDS; c <= 128, (k - 1) / 2 * (d0 + d1) <= 64 rows) or by two `efts_gemm` launches ((k - 1) * d <= 64 rows each); `ps.fused` says which."""

    def __init__(self, channels: int, kernel_size: int, dilation):
        super().__init__()
        self.convs = _weight_normed(channels, kernel_size, dilation[:2])
        self.kernel_size, self.dilation = kernel_size, tuple(dilation[:2])

    @staticmethod
    def fusable(c: int, k: int, ds) -> bool:            # one efts_resblock2 launch can run this geometry
        return c <= _RB2_MAX_C and k in _RB2_TAPS and (k - 1) // 2 * (ds[0] + ds[1]) <= _RB2_MAX_HALO

    @staticmethod
    def composable(k: int, ds) -> bool:                 # two efts_gemm launches can run this geometry
        return k in _GEMM_TAPS and all((k - 1) * d <= _GEMM_MAX_SPAN for d in ds)

    @staticmethod
    def refusal(k: int, ds, c_max: int) -> Optional[str]:
        """why neither the fused launch nor two efts_gemm launches can run a block of this geometry at up to c_max channels"""
        if len(ds) != 2:
            return (f"resblock '2' with {len(ds)} dilations for kernel size {k}: the reference's ResBlock2 uses exactly dilation[0] and "
                    "dilation[1] (a list of three is a ResBlock1 configuration)")
        if min(ds) < 1:
            return _bad_dilation(k, next(d for d in ds if d < 1))
        if _ResBlock2.composable(k, ds) or _ResBlock2.fusable(c_max, k, ds):
            return None
        why = f"ResBlock2 with kernel size {k} and dilations {list(ds)}"    # a window span above 64 rows: only the fused launch, in every stage
        if c_max > _RB2_MAX_C:
            return f"{why} at {c_max} channels: (k - 1) * d above {_GEMM_MAX_SPAN} rows is beyond efts_gemm, and efts_resblock2 takes c <= {_RB2_MAX_C}"
        return (f"{why}: (k - 1) * d above {_GEMM_MAX_SPAN} rows is beyond efts_gemm, and efts_resblock2 takes (k - 1) / 2 * (d0 + d1) <= "
                f"{_RB2_MAX_HALO} rows")

    def packed(self, n: int):           # (packed name, module) of block n in launch order
        return [(f"rb{n}.c.{d}", m) for d, m in enumerate(self.convs)]

    @staticmethod
    def scratch(chains: int, rows: int, c: int, split: int, dev):     # per chain: the ping-pong pair (the composed arm's intermediate, the result)
        return [[_Rows(rows, c, split, dev) for _ in range(2)] for _ in range(chains)]

    def launch(self, ps: _Pass, n: int, up: _Up, pp, key: str) -> int:
        """block n on the current stream (:81-88): the pointer of the fp32 result (pp[1]); keeps it as "{key}" """
        c0, c1, k, ds, c = ps.pk[f"rb{n}.c.0"], ps.pk[f"rb{n}.c.1"], self.kernel_size, self.dilation, up.c
        if ps.fused(c, k, ds):
            g = L.ResBlock2Args()
            g.x, g.ldx, g.p0, g.ldp, g.rowmask, g.out, g.ldo = up.x_f, c, up.x_p.ptr, up.x_p.ld, up.mask.data_ptr(), pp[1].fptr, c
            g.w0, g.w1, g.ldw, g.w_tap_stride = c0.w.ptr, c1.w.ptr, c0.w.ld, c0.w.tap_stride
            g.bias0, g.bias1 = c0.bias.data_ptr(), c1.bias.data_ptr()
            g.split, g.m, g.c, g.k, g.d0, g.d1, g.slope = ps.split, up.rows, c, k, ds[0], ds[1], LRELU_SLOPE
            L.check(L.load().efts_resblock2(ctypes.byref(g), O._stream()), "efts_resblock2")
        else:       # one efts_gemm launch per turn: the first also writes the operand plane of leaky(y1) for the second
            _conv(c0, up.x_p, up.rows, k, ds[0], mask=up.mask, out_f=pp[0].fptr, ldo=c, out_p=pp[0].p, plane_slope=LRELU_SLOPE,
                  resid=up.x_f, ldr=c)
            _conv(c1, pp[0].p, up.rows, k, ds[1], mask=up.mask, out_f=pp[1].fptr, ldo=c, resid=pp[0].fptr, ldr=c)
        if ps.keep is not None:
            ps.keep[key] = pp[1].f.clone()
        return pp[1].fptr


_BLOCKS = {"1": _ResBlock1, "2": _ResBlock2}


class _TanhHead:
    """HiFi-GAN's head (hifigan_model.py:130-131): conv_post to one channel with the kernel's tanh epilogue, the items copied out of the row space"""
    channels, samples_per_row, writes_silence, tag = 1, 1, False, ()

    @staticmethod
    def tables(dev) -> None:                    # no constants
        return None

    @staticmethod
    def scratch(rows: int, dev):                # the fp32 column of the whole row space
        return torch.zeros(rows + 256, 1, dtype=torch.float32, device=dev)

    def launch(self, ps: _Pass, cur: _Act, mask: torch.Tensor, audio: torch.Tensor) -> None:
        out = ps.ws.head
        _conv(ps.pk["conv_post"], cur.p, cur.rows, 7, 1, mask=mask, out_f=out.data_ptr(), ldo=1, act=L.ACT_TANH)
        audio[:, 0].copy_(out[:cur.rows, 0].view(ps.B, ps.pitch * ps.rate)[:, :ps.T * ps.rate])
        if ps.keep is not None:
            ps.keep["out"] = out.clone()


class _IstftHead:
    """iSTFTNet's head (include/efts_abi.h "The head of an iSTFTNet generator"): conv_post emits a log-magnitude and a phase argument per bin of
    an N-point STFT for L + 1 frames per item, frame 0 on the reflected row a'[0] = a[1]; the inverse STFT with hop N / 4 makes the samples.
    Three launches: the reflected row is copied one row in front of every item of the last stage's `s` plane (the guard rows for item 0, the gap
    rows for the others; nothing but conv_post reads that plane), conv_post reads the plane from one row further up, `efts_istft_head` writes
    the audio, silence past every length included.  The window and the twiddle table are constants, built in float64; no parameters."""
    writes_silence = True

    def __init__(self, n_fft: int, hop: int):
        self.n_fft, self.hop = n_fft, hop
        self.channels, self.samples_per_row = n_fft + 2, hop
        self._tables = {}                       # device -> fp32 [3 N]: window, then (cos, sin)(2 pi j / N) interleaved

    @staticmethod
    def refusal(n_fft, hop) -> Optional[str]:
        if n_fft is None:
            return None if hop is None else "gen_istft_hop_size without gen_istft_n_fft: the hop belongs to an iSTFT head, which gen_istft_n_fft asks for"
        if n_fft not in _ISTFT_N:
            return f"gen_istft_n_fft {n_fft}: efts_istft_head takes {', '.join(map(str, _ISTFT_N))}"
        if hop is None or hop * 4 != n_fft:
            return f"gen_istft_hop_size {hop} with gen_istft_n_fft {n_fft}: efts_istft_head overlaps four frames, hop = n_fft / 4 = {n_fft // 4}"
        return None

    def tables(self, dev) -> torch.Tensor:
        if dev not in self._tables:
            ang = 2.0 * math.pi * torch.arange(self.n_fft, dtype=torch.float64) / self.n_fft
            self._tables[dev] = torch.cat([0.5 - 0.5 * torch.cos(ang), torch.stack([torch.cos(ang), torch.sin(ang)], 1).flatten()]).float().to(dev)
        return self._tables[dev]

    @property
    def tag(self):
        return ("istft", self.n_fft, self.hop, tuple(t.data_ptr() for t in self._tables.values()))

    def scratch(self, rows: int, dev):          # z: conv_post's fp32 result, frame f of item b at row b * pitch + f; the mask of the L + 1 frames
        return (torch.zeros(rows + 2, self.channels, dtype=torch.float32, device=dev), torch.zeros(rows + 1, dtype=torch.float32, device=dev))

    def launch(self, ps: _Pass, cur: _Act, mask: torch.Tensor, audio: torch.Tensor) -> None:
        (z, fmask), tab, lib, rows_item = ps.ws.head, self.tables(ps.dev), L.load(), ps.pitch * ps.rate
        rows = ps.lens * ps.rate
        frames = torch.where(rows > 0, rows + 1, rows)
        L.check(lib.efts_row_masks(frames.data_ptr(), None, fmask.data_ptr(), ps.B, ps.T * ps.rate + 1, rows_item, ps.st), "efts_row_masks")
        g = L.IstftHeadArgs()
        g.mode, g.B, g.pitch, g.plane, g.ld_plane = L.ISTFT_REFLECT, ps.B, rows_item, cur.p.ptr, cur.p.ld
        L.check(lib.efts_istft_head(ctypes.byref(g), ps.st), "efts_istft_head")
        # row r of z is centred on row r - 1 of the plane: a' of item b begins one row in front of the item
        _conv(ps.pk["conv_post"], cur.p, cur.rows, 7, 1, mask=fmask, out_f=z.data_ptr(), ldo=self.channels, a_ptr=cur.p.ptr - cur.p.ld)
        g = L.IstftHeadArgs()
        g.mode, g.B, g.pitch, g.z, g.z_rows, g.lengths, g.len_mul = L.ISTFT_SYNTH, ps.B, rows_item, z.data_ptr(), cur.rows, ps.lens.data_ptr(), ps.rate
        g.window, g.twiddle, g.n_fft, g.hop = tab.data_ptr(), tab.data_ptr() + 4 * self.n_fft, self.n_fft, self.hop
        g.audio, g.ld_audio, g.out_len = audio.data_ptr(), audio.shape[2], audio.shape[2]
        L.check(lib.efts_istft_head(ctypes.byref(g), ps.st), "efts_istft_head")
        if ps.keep is not None:
            ps.keep["z"], ps.keep["out"] = z.clone(), audio.clone()


def _refusal(rates, kernels, res_kernels, res_dilations, c0, num_mels, resblock: str = "1", istft_n_fft=None, istft_hop=None) -> Optional[str]:
    """why the launches of the stages cannot compute this configuration (None: they can)"""
    why = _IstftHead.refusal(istft_n_fft, istft_hop)
    if why is not None:
        return why
    if resblock not in _BLOCKS:
        return f"resblock {resblock!r}: the reference has ResBlock1 ('1') and ResBlock2 ('2')"
    if not rates or len(rates) != len(kernels):
        return "upsample_rates and upsample_kernel_sizes must be non-empty lists of one length"
    for u, k in zip(rates, kernels):
        if u <= 0 or k != 2 * u or u % 2:
            return "transposed convolutions are implemented for kernel = 2 * stride, even stride"
    if not 1 <= len(res_kernels) <= _MAX_RES_KERNELS:
        return (f"{len(res_kernels)} resblock_kernel_sizes: the multi-receptive-field mean (efts_mean_act_rows) adds one to "
                f"{_MAX_RES_KERNELS} residual chains")
    if len(res_dilations) != len(res_kernels):
        return "resblock_dilation_sizes must hold one list per entry of resblock_kernel_sizes"
    for k, ds in zip(res_kernels, res_dilations):
        if k not in _GEMM_TAPS:
            return f"residual kernel size {k}: efts_gemm takes {', '.join(map(str, _GEMM_TAPS))} taps"
        if not ds:
            return "an empty dilation list (a residual block without convolutions) is not implemented"
        why = _BLOCKS[resblock].refusal(k, ds, c0 // 2 if c0 > 0 else 0)      # the widest stage is the first
        if why is not None:
            return why
    c_last = c0 // 2 ** len(rates)
    if c0 <= 0 or c0 % 2 ** len(rates) or c_last % 4:
        return (f"upsample_initial_channel {c0} over {len(rates)} stages: every stage needs a whole channel count that is a multiple "
                "of 4 (the 4-column accesses of the elementwise kernels)")
    if not 1 <= num_mels <= 4096:
        return "num_mels must be in 1 .. 4096 (efts_pack_rows)"
    return None


class HiFiGANGenerator(nn.Module):
    def __init__(self, h, precision: str = "bf16x3"):
        super().__init__()
        self.resblock = str(_cfg(h, "resblock", "1"))
        splits = {"bf16": L.SPLIT_BF16, "bf16x3": L.SPLIT_BF16X3, "fp32": L.SPLIT_FP32}     # fp32: exact operands, generic efts_gemm tiling
        if precision not in splits:
            raise ValueError("precision must be 'bf16x3', 'bf16' or 'fp32'")
        self.precision, self.split = precision, splits[precision]
        self.upsample_rates = tuple(_cfg(h, "upsample_rates"))
        self.upsample_kernel_sizes = tuple(_cfg(h, "upsample_kernel_sizes"))
        self.res_kernels = tuple(_cfg(h, "resblock_kernel_sizes"))
        self.res_dilations = tuple(tuple(d) for d in _cfg(h, "resblock_dilation_sizes"))
        c0 = int(_cfg(h, "upsample_initial_channel"))
        self.num_mels = int(_cfg(h, "num_mels", 80))
        n_fft, istft_hop = _cfg(h, "gen_istft_n_fft"), _cfg(h, "gen_istft_hop_size")
        why = _refusal(self.upsample_rates, self.upsample_kernel_sizes, self.res_kernels, self.res_dilations, c0, self.num_mels,
                       self.resblock, n_fft, istft_hop)
        if why is not None:
            raise NotImplementedError(why)
        self.gap_frames = gap_frames(self.upsample_rates, self.res_kernels, self.res_dilations)
        self._rates = [math.prod(self.upsample_rates[:i]) for i in range(len(self.upsample_rates) + 1)]    # samples per mel frame in front of stage i
        self._head = _TanhHead() if n_fft is None else _IstftHead(int(n_fft), int(istft_hop))       # (no module: a head has no parameters)
        self.hop = self._rates[-1] * self._head.samples_per_row         # samples per mel frame
        self._chain_order = sorted(range(len(self.res_kernels)), key=lambda j: -self.res_kernels[j])   # the longest chain is issued first
        self.conv_pre = weight_norm(nn.Conv1d(self.num_mels, c0, 7, 1, padding=3))
        self.ups = nn.ModuleList([weight_norm(nn.ConvTranspose1d(c0 // 2 ** i, c0 // 2 ** (i + 1), k, u, padding=(k - u) // 2))
                                  for i, (u, k) in enumerate(zip(self.upsample_rates, self.upsample_kernel_sizes))])
        self.resblocks = nn.ModuleList([_BLOCKS[self.resblock](m.out_channels, k, d) for m in self.ups
                                        for k, d in zip(self.res_kernels, self.res_dilations)])
        self.conv_post = weight_norm(nn.Conv1d(self.ups[-1].out_channels, self._head.channels, 7, 1, padding=3))
        self._packed, self._packed_dev = None, None             # Dict[str, _Conv] and the device it was packed for
        self._bufs, self._bstreams = Cache(capacity=3), []      # (B, T) -> _Workspace; the side streams of the residual chains
        # per-shape hipGraph of the ~85 launches of a call (round 6; efficient_tts_amd/graphs.py, the acoustic model's cache): one utterance is
        # 2 ms of device work issued by a host that needs about as long for the launches; `graphs = False`: every launch issued eagerly
        self.graphs = True
        # ResBlock2: True = the fused launch wherever it can run, two efts_gemm launches for the rest; False = the reverse.  Measured (tools/micro/
        # vocoder_rb2_timing.py): V3 at one 800-frame utterance 0.87 ms fused, 0.74 ms composed; 4.79 and 3.95 ms at a batch of 8: the default composes
        self.fused_resblock2 = False
        self.branch_streams = True          # the residual blocks of a stage on streams of their own (False: one after the other, A/B)
        from .graphs import GraphCache
        object.__setattr__(self, "_graph_cache", GraphCache(capacity=4))

    # ------------------------------------------------------------------ reference API
    def remove_weight_norm(self):
        self._graph_cache.clear()
        for m in [self.conv_pre, self.conv_post, *self.ups, *(m for n, rb in enumerate(self.resblocks) for _, m in rb.packed(n))]:
            remove_weight_norm(m)
        self._packed = None

    def load_state_dict(self, *a, **k):
        self._packed = None
        self._graph_cache.clear()
        return super().load_state_dict(*a, **k)

    # ------------------------------------------------------------------ weights -> operand planes (once)
    @staticmethod
    def _folded(m: nn.Module) -> torch.Tensor:
        if hasattr(m, "weight_g"):
            # weight_norm, dim 0 (Conv1d: per cout; ConvTranspose1d: per cin) -- the very op remove_weight_norm bakes in
            return torch._weight_norm(m.weight_v.detach(), m.weight_g.detach(), 0)
        return m.weight.detach()

    def _pack(self, dev) -> Dict[str, _Conv]:
        if self._packed is not None and self._packed_dev == dev:
            return self._packed
        self._bufs.clear()                      # workspaces of another device are of no use either
        self._packed_dev = dev
        pk: Dict[str, _Conv] = {}
        with O.stream_scope():
            def conv(name, m):
                w = self._folded(m).float().contiguous()
                pw = PackedWeight(w.shape[0], w.shape[1], w.shape[2], self.split, dev)
                pw.pack(w)
                pk[name] = _Conv(pw, m.bias.detach().float().contiguous())
            conv("conv_pre", self.conv_pre)
            conv("conv_post", self.conv_post)
            for i, (m, u) in enumerate(zip(self.ups, self.upsample_rates)):
                w = self._folded(m).float()                                  # [cin][cout][2u]
                cin, cout, _ = w.shape
                # B[tap][n = r * cout + co][ci]: tap 0 multiplies x[q-1] (w[.., r + u]), tap 1 multiplies x[q] (w[.., r]), tap 2 = 0
                b = torch.zeros(u * cout, cin, 3, device=dev)
                b[:, :, 0] = w[:, :, u:].permute(2, 1, 0).reshape(u * cout, cin)
                b[:, :, 1] = w[:, :, :u].permute(2, 1, 0).reshape(u * cout, cin)
                pw = PackedWeight(u * cout, cin, 3, self.split, dev)
                pw.pack(b.contiguous())
                pk[f"ups.{i}"] = _Conv(pw, m.bias.detach().float().repeat(u).contiguous())
            for n, rb in enumerate(self.resblocks):
                for name, m in rb.packed(n):
                    conv(name, m)
        self._packed = pk
        return pk

    # ------------------------------------------------------------------ buffers per mel length
    def _workspace_for(self, B: int, T: int, dev) -> _Workspace:
        return self._bufs.get((B, T), lambda: self._make_workspace(B, T, dev))

    def _make_workspace(self, B: int, T: int, dev) -> _Workspace:
        sp, pitch = self.split, T + self.gap_frames                            # pitch: rows per item at mel rate
        rows = B * pitch
        mel = _Rows(rows, self.num_mels, sp, dev, f32=False)
        pre = _Rows(rows, self.conv_pre.out_channels, sp, dev, f32=False)
        stages = []
        for m, u in zip(self.ups, self.upsample_rates):
            c, n_i = m.out_channels, rows * u
            stages.append(_Stage(up=_Rows((rows + 1) * u, c, sp, dev, plane=False),   # the [rows + 1][u * c] GEMM result, seen as rows of c
                                 x=_Rows(n_i, c, sp, dev, f32=False), chains=_BLOCKS[self.resblock].scratch(len(self.res_kernels), n_i, c, sp, dev),
                                 s=_Rows(n_i, c, sp, dev, f32=False),
                                 mask=torch.zeros(n_i + 1, dtype=torch.float32, device=dev)))
            rows = n_i
        return _Workspace(pitch, mel, pre, stages, mask_mel=torch.zeros(B * pitch + 1, dtype=torch.float32, device=dev),
                          head=self._head.scratch(rows, dev))

    def _branch_streams(self, dev, count: int):
        if len(self._bstreams) != count or (count and self._bstreams[0].device != dev):
            self._bstreams = [torch.cuda.Stream(device=dev) for _ in range(count)]
        return self._bstreams

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, x: torch.Tensor, lengths: Optional[torch.Tensor] = None, keep: Optional[dict] = None) -> torch.Tensor:
        """mel [B, num_mels, T] -> audio [B, 1, T * hop].  `lengths` (frames per item, optional): every item is synthesised exactly as if it had been
        passed alone without its padding; samples past lengths[b] * hop are 0.  `keep` (a dict, for the tests; like `_forward_impl(..., keep=True)` of
        the acoustic model): every step's output buffer is cloned into it (`_run`); eagerly issued launches only: `graphs = False`, never under capture."""
        if x.dim() != 3 or x.shape[1] != self.num_mels:
            raise ValueError(f"expected mel [B, {self.num_mels}, T]")
        if not x.is_cuda:
            raise RuntimeError("HiFiGANGenerator runs on an MI355X device only (no CPU path)")
        L.load()
        L.require_device()
        dev = x.device
        pk = self._pack(dev)
        self._head.tables(dev)                  # (constants of the head on the device, made once, outside any capture)
        B, _, T = x.shape
        lens = torch.full((B,), T, dtype=torch.int32, device=dev) if lengths is None else lengths.to(device=dev, dtype=torch.int32).clamp(0, T)
        mel = x.transpose(1, 2).float()
        if lengths is not None:                 # what the padding frames hold must not reach conv_pre's halo
            mel = mel * (torch.arange(T, device=dev)[None, :] < lens[:, None])[:, :, None]
        mel = mel.contiguous()

        def body(mel_btc, lens_i32):
            audio = (torch.empty if self._head.writes_silence else torch.zeros)(B, 1, T * self.hop, dtype=torch.float32, device=dev)
            with O.stream_scope():
                ws = self._workspace_for(B, T, dev)
                self._run(_Pass(ws=ws, pk=pk, B=B, T=T, pitch=ws.pitch, rate=self._rates[-1], lens=lens_i32, dev=dev, st=O._stream(),
                                split=self.split, fused=self._rb2_fused, keep=keep), mel_btc, audio)
            return (audio,)

        if keep is not None and (self.graphs or torch.cuda.is_current_stream_capturing()):
            raise RuntimeError("keep: the stages are observed on eagerly issued launches only (graphs = False, no capture)")
        if not self.graphs or torch.cuda.is_current_stream_capturing():
            return body(mel, lens)[0]
        ws = self._workspace_for(B, T, dev)
        # the graph is valid while the buffers its launches point at live: this workspace and the packed planes
        tag = (id(ws), tuple(cv.w.ptr for cv in pk.values()), self.split, self.fused_resblock2) + self._head.tag
        return self._graph_cache.run(("voc", B, T), tag, (mel, lens), body, keepalive=(ws, pk, self._head), adaptive=True)[0]

    def _rb2_fused(self, c: int, k: int, ds) -> bool:   # which arm runs a ResBlock2 of this geometry (the constructor refused what neither can)
        return _ResBlock2.fusable(c, k, ds) if self.fused_resblock2 else not _ResBlock2.composable(k, ds)

    def _run(self, ps: _Pass, mel_btc: torch.Tensor, audio: torch.Tensor) -> None:
        """ps.keep (None: nothing happens): after each step a clone of what it wrote, made on the stream of the step's launch and complete when `_run`
        returns (it ends with a device synchronisation then).  Whole buffers, guard rows included: "pre", "x{i}", "s{i}" operand planes (uint8
        [alloc][ld], row 0 at _GUARD); "r{i}.{j}.{d}" fp32 [alloc][c] of residual block j after pair d (ResBlock2: "r{i}.{j}", the block's fp32
        output); "up{i}" fp32 [rows][c] behind the u / 2-row offset; "out" fp32 [rows + 256][1]; "pitch": rows per item at mel rate.  An iSTFT
        head: "z" fp32 [rows + 2][N + 2], conv_post's result with frame f of item b at row b * pitch * rate + f, and "out", the audio."""
        cur = self._stage_pre(ps, mel_btc)
        for i in range(len(self.ups)):
            up = self._stage_upsample(ps, i, cur)
            cur = self._stage_mean(ps, i, up, self._stage_residual(ps, i, up))
        self._stage_post(ps, cur, audio)
        if ps.keep is not None:
            torch.cuda.synchronize(ps.dev)              # the side streams' clones included

    def _stage_pre(self, ps: _Pass, mel_btc: torch.Tensor) -> _Act:
        ws, mel_p, rows = ps.ws, ps.ws.mel.p, ps.B * ps.pitch
        L.check(L.load().efts_pack_rows(mel_btc.data_ptr(), None, mel_p.ptr, mel_p.ld, ps.B, ps.T, ps.pitch, self.num_mels,
                                        mel_p.nchunk * O.chunk_k(ps.split), ps.split, ps.st), "efts_pack_rows")
        L.check(L.load().efts_row_masks(ps.lens.data_ptr(), None, ws.mask_mel.data_ptr(), ps.B, ps.T, ps.pitch, ps.st), "efts_row_masks")
        _conv(ps.pk["conv_pre"], mel_p, rows, 7, 1, mask=ws.mask_mel, out_p=ws.pre.p, plane_slope=LRELU_SLOPE)      # :118 (+ :120)
        if ps.keep is not None:
            ps.keep["pitch"], ps.keep["pre"] = ps.pitch, ws.pre.p.buf.clone()
        return _Act(ws.pre.p, rows)

    def _stage_upsample(self, ps: _Pass, i: int, cur: _Act) -> _Up:
        sg, u, c, rate = ps.ws.stages[i], self.upsample_rates[i], self.ups[i].out_channels, self._rates[i + 1]
        n_i, lens = cur.rows * u, ps.lens * rate
        L.check(L.load().efts_row_masks(lens.data_ptr(), None, sg.mask.data_ptr(), ps.B, ps.T * rate, ps.pitch * rate, ps.st), "efts_row_masks")
        # ConvTranspose1d as a 2-tap convolution over the input rows + 1 (the row after the last one is a zero guard row)
        _conv(ps.pk[f"ups.{i}"], cur.p, cur.rows + 1, 3, 1, out_f=sg.up.fptr, ldo=u * c)
        x_f, x_p = sg.up.fptr + (u // 2) * c * 4, sg.x.p                   # y[n] = row n + u/2 of the flattened result
        # plane of leaky(x): x * (x > 0 ? 1 : slope), the identity-residual LeakyReLU mode of efts_act_bwd; the mask drops
        # the transposed convolution's cropped border samples, which land in the zero rows between items
        L.check(L.load().efts_act_bwd(x_f, x_f, None, sg.mask.data_ptr(), LRELU_SLOPE, 3, None, x_p.ptr, x_p.ld, ps.split, None, n_i, c,
                                      ps.st), "efts_act_bwd")
        if ps.keep is not None:
            lo = (_GUARD + u // 2) * c
            ps.keep[f"up{i}"], ps.keep[f"x{i}"] = sg.up.f.view(-1)[lo:lo + n_i * c].view(n_i, c).clone(), x_p.buf.clone()
        return _Up(x_f, x_p, sg.mask, n_i, c)

    def _stage_residual(self, ps: _Pass, i: int, up: _Up) -> List[int]:
        """The residual blocks of a stage are independent until their mean (:123-128): each runs as a chain of its own on its own stream (round 6).
        At one utterance a launch is 50-200 workgroups for 15-30 us: eighteen of them in a row per stage were latency, not work
        (profiles/rocprofv3_r06_vocoder_summary.txt); two chains' workgroups fit a CU's LDS side by side.  Returns each block's fp32 result."""
        nk = len(self.res_kernels)
        main = torch.cuda.current_stream(ps.dev)
        side = self._branch_streams(ps.dev, nk - 1) if self.branch_streams else []
        ev_x = O.hand_over(main)
        finals, joins = [0] * nk, []
        for slot, j in enumerate(self._chain_order):
            own = side[slot] if slot < len(side) else None              # the last (shortest) chain stays on the main stream
            if own is not None:
                own.wait_event(ev_x)
            with (O.on_stream(own) if own is not None else contextlib.nullcontext()):
                finals[j] = self.resblocks[i * nk + j].launch(ps, i * nk + j, up, ps.ws.stages[i].chains[j], f"r{i}.{j}")
                if own is not None:
                    joins.append(O.hand_over(own))
        for ev in joins:
            main.wait_event(ev)
        return finals

    def _stage_mean(self, ps: _Pass, i: int, up: _Up, finals: List[int]) -> _Act:
        s_p, (f0, f1, f2) = ps.ws.stages[i].s.p, (finals + [None, None])[:3]
        slope = 0.01 if i == len(self.ups) - 1 else LRELU_SLOPE              # :128 (+ :120 / :129)
        L.check(L.load().efts_mean_act_rows(f0, f1, f2, up.c, 1.0 / len(finals), slope, None, 0, s_p.ptr, s_p.ld, ps.split, up.rows, up.c,
                                            ps.st), "efts_mean_act_rows")
        if ps.keep is not None:
            ps.keep[f"s{i}"] = s_p.buf.clone()
        return _Act(s_p, up.rows)

    def _stage_post(self, ps: _Pass, cur: _Act, audio: torch.Tensor) -> None:      # the head: `_TanhHead` (:130-131) or `_IstftHead`
        self._head.launch(ps, cur, ps.ws.stages[-1].mask, audio)


def load_hifigan_generator(device, config_path: str, checkpoint_path: str, precision: str = "bf16x3") -> HiFiGANGenerator:
    """The reference's loader (hifigan_model.py:18-28) with explicit paths: JSON config + a checkpoint whose "generator" entry is the reference
    Generator's state_dict (the published `generator_v1` is not shipped with the reference repository)."""
    import json
    with open(config_path) as f:
        cfg = json.load(f)
    gen = HiFiGANGenerator(cfg, precision=precision)
    state = torch.load(checkpoint_path, map_location="cpu")
    gen.load_state_dict(state["generator"] if "generator" in state else state)
    gen = gen.to(device).eval()
    gen.remove_weight_norm()
    return gen
